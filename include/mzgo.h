/* mzgo.h -- C ABI of the MI355X-native MuZero-Go self-play engine (libmzgo.so).
 *
 * The reference (Sir-Teo/MuZero-Go) is pure Python with no FFI; its hot path
 * is reached through duck-typed protocols.  Each entry point below replaces
 * one of them (citations are into the reference snapshot):
 *
 *   mzgo_initial_inference    MuZeroNet.initial_inference      self_play.py:121-124
 *   mzgo_recurrent_inference  MuZeroNet.recurrent_inference    self_play.py:125-128
 *   mzgo_set_weights          MuZeroNet.load_state_dict /       self_play.py:404-412
 *                             MuZeroAgent.load_weights
 *   mzgo_set_weights_device   the same from the parameters in device memory
 *                             (after an optimizer step; no reference counterpart)
 *   mzgo_search               MCTS.run                         self_play.py:148-237
 *   mzgo_board_reset          GoEnv.reset (GymGo)              self_play.py:455
 *   mzgo_board_step           GoEnv.step  (GymGo)              self_play.py:479
 *   mzgo_board_planes         the observation array GoEnv returns
 *   mzgo_selfplay_move        one iteration of run_self_play_game's loop,
 *                             for every game slot              self_play.py:465-507
 *   mzgo_records_export       GameHistory / the pickle writer  self_play.py:415-450, :561-583
 *   mzgo_optim_step           clip_grad_norm_ + Adam.step +    main.py:481-484, :379
 *                             StepLR.step over the parameters
 *
 * Conventions
 *   - All tensor arguments are DEVICE pointers (hipMalloc / torch CUDA tensors)
 *     unless the name ends in _host.  Shapes are C-contiguous.
 *   - ``stream`` is a hipStream_t (NULL = the null stream).  Calls enqueue work
 *     and return; nothing synchronises unless documented.
 *   - Return value: 0 on success, a negative MZGO_E* code on failure;
 *     mzgo_last_error() then describes it (thread-local).
 *   - An engine is not thread-safe.
 *   - Actions are row-major cells a = r*N + c, pass = N*N (GymGo's flattening).
 *   - Observation planes are [6][N][N]: BLACK, WHITE, TURN, INVD, PASS, DONE.
 */
#ifndef MZGO_H
#define MZGO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MZGO_OK = 0,
  MZGO_EINVAL = -1,      /* bad argument / unsupported configuration */
  MZGO_EHIP = -2,        /* HIP runtime error */
  MZGO_ENOWEIGHTS = -3,  /* network weights incomplete */
  MZGO_EASSERT = -4      /* GymGo assertion (invalid move, step after done) */
};

typedef struct mzgo_config {
  int board_size;           /* N: 5, 6, 9 or 19 (self_play.py:20) */
  int latent_dim;           /* C: 96 (self_play.py:21); 0 = board-only engine */
  int num_games;            /* G: game slots held on the device */
  int num_simulations;      /* S: MCTS simulations per move (self_play.py:23) */
  int max_moves;            /* move cap, N*N in the reference (self_play.py:461); 0 = N*N */
  int compat;               /* 0 = reference (zero visit counts, §0.6), 1 = fixed */
  int temperature_moves;    /* 15 (self_play.py:29) */
  int search_variant;       /* 0 = self_play.py's MCTS (:142-343), 1 = main.py's MCTS
                               (main.py:246-368: trainer self-play and arena rules) */
  double c_puct;            /* 2.5 (self_play.py:143); main.py's variant uses 2 */
  double discount;          /* 0.99 */
  double dirichlet_alpha;   /* 0.15 */
  double dirichlet_epsilon; /* 0.02 */
  double pass_epsilon;      /* 0.01 */
  double temperature;       /* 1.0 */
  double komi;              /* 0 (self_play.py:544) */
  uint64_t seed;            /* counter-RNG seed */
  int game_base;            /* global id of slot 0 (multi-GPU game sharding) */
  int device;               /* HIP device ordinal */
  int direct_dynamics;      /* 0 = factored expansion (default): a search convolves each
                               parent once and expands children as relu(Y + E[a]), exact
                               up to fp32 rounding (see muzero-go_amd/csrc/mzgo_expand.hpp);
                               1 = one dynamics conv per simulation, as the reference does */
  int tower;                /* 0 = the reference network (self_play.py:63-128); 1 = the
                               residual-tower network of BASELINE config 5 (mzgo/resnet.py:
                               conv_in + res_blocks residual blocks in the representation and
                               the dynamics, the reference's heads), bf16 MFMA with fp32
                               accumulation, latent_dim a multiple of 64, N in {5, 9, 19} */
  int res_blocks;           /* residual blocks per tower network (tower = 1) */
  int fast_simulations;     /* playout cap randomization (KataGo): 0 = off (default); F in
                               1..num_simulations = a self-play move is searched with F
                               simulations instead of num_simulations with probability
                               1 - full_search_prob, and its record's flags carry bit3.  A
                               fast search is the same search with fewer simulations (same
                               noise, temperature and move rule).  Self-play moves only
                               (mzgo_selfplay_move(s), mzgo_replay_play_games): mzgo_search,
                               mzgo_reanalyse, mzgo_replay_reanalyse* and the arena always
                               search with num_simulations.  Refused on tower engines;
                               board-only engines ignore it */
  double full_search_prob;  /* probability of a full search, in [0, 1]; default 1.0.  The
                               choice is mzgo_playout_budget_host's, a pure function of
                               (seed, key game id, move) */
} mzgo_config;

typedef struct mzgo_engine mzgo_engine;

/* Fill *cfg with the reference defaults (self_play.py:19-33) for board size N. */
void mzgo_default_config(mzgo_config* cfg, int board_size);

int mzgo_engine_create(const mzgo_config* cfg, mzgo_engine** out);
void mzgo_engine_destroy(mzgo_engine* eng);
/* The simulations of self-play move `move` of the game with key id key_gid
 * ((game_base + g) ^ (epoch << 24)) under playout cap randomization -- the
 * function the self-play kernels run, on the host, no device work:
 *   *budget = num_simulations                  if fast_simulations == 0
 *           = num_simulations                  if u01(draw(stream_key(seed, key_gid, move), 8, 0)) < full_search_prob
 *           = fast_simulations                 otherwise
 * u01 is in [0, 1): full_search_prob 1.0 is always full, 0.0 always fast.
 * MZGO_EINVAL for a null budget, num_simulations < 1, fast_simulations
 * outside 0..num_simulations, move < 0 or full_search_prob outside [0, 1]. */
int mzgo_playout_budget_host(uint64_t seed, uint32_t key_gid, int move, int num_simulations, int fast_simulations,
                             double full_search_prob, int* budget);
const char* mzgo_last_error(void);
/* Bytes of device memory the engine owns. */
int64_t mzgo_engine_device_bytes(const mzgo_engine* eng);

/* Load one state_dict tensor (host float32, reference key and shape, e.g.
 * "dynamics.conv.weight" (C,C,3,3)); packed into MFMA fragment order on upload.
 * mzgo_weights_ready() returns 1 once all 22 keys are loaded. */
int mzgo_set_weights(mzgo_engine* eng, const char* key, const float* data_host,
                     const int64_t* shape, int ndim);
int mzgo_weights_ready(const mzgo_engine* eng);

/* The same weights from device memory (reference network engines, tower = 0).
 *
 * All 22 state_dict tensors from device memory (float32, contiguous, on the
 * engine's device), packed on `stream` by kernels; no host copy is made.
 * keys/data/shapes/ndims have n entries and must name every key exactly once.
 * The embedding is (N*N+1, C): the first rows of a larger table.
 *
 * Ordering: the pack is enqueued on `stream` and returns without waiting.  It
 * reads the tensors and writes the engine's packed weights in stream order, so
 * (as for every other entry point) calls on one engine share a stream or are
 * synchronised by the caller: the tensors must not change before the pack has
 * run, and no launch of this engine on another stream may still be running or
 * start before it has.  After the first load of an engine (which allocates),
 * mzgo_set_weights_device and mzgo_weights_copy allocate nothing, make no
 * blocking copy and synchronise neither stream nor device.
 *
 * Afterwards the engine's host copies (mzgo_set_weights) are dropped:
 * mzgo_weights_ready() returns 1, and a later mzgo_set_weights takes effect
 * once all 22 keys have been given again (MZGO_ENOWEIGHTS until then). */
int mzgo_set_weights_device(mzgo_engine* eng, const char* const* keys, const float* const* data_dev,
                            const int64_t* const* shapes, const int* ndims, int n, void* stream);
/* dst's packed weights := src's (same board_size, latent_dim, tower = 0): one
 * device-to-device copy on `stream`.  Tensors that src got by mzgo_set_weights
 * and has not uploaded yet are packed first (that part blocks, as every first
 * use after mzgo_set_weights does). */
int mzgo_weights_copy(mzgo_engine* dst, const mzgo_engine* src, void* stream);
/* The packed blob to the host (synchronises `stream`): *n_floats = its length;
 * data may be NULL to query; cap in floats.  A test and diagnostic hook: the
 * layout is mzgo_weights.hpp's and depends on (board_size, latent_dim) only. */
int mzgo_weights_export(mzgo_engine* eng, float* data_host, int64_t cap, int64_t* n_floats, void* stream);
/* The blob's host twin: the packed blob of a (board_size, latent_dim) engine
 * from the 22 state_dict tensors in host memory (mzgo_set_weights_device's
 * table and its checks), by a serial walk of the rules the pack kernel runs --
 * the same floats bit for bit, without an engine, a device or a HIP call.
 * *n_floats = the blob's length; blob may be NULL to query; cap in floats.
 * MZGO_EINVAL for a (board_size, latent_dim) no kernels are built for. */
int mzgo_weights_pack_host(int board_size, int latent_dim, const char* const* keys, const float* const* data_host,
                           const int64_t* const* shapes, const int* ndims, int n, float* blob, int64_t cap,
                           int64_t* n_floats);

/* MuZeroNet protocol, batch B (any B >= 1):
 *   obs f32 [B][6][N][N] -> latent f32 [B][C][N][N], value f32 [B][1], logits f32 [B][N*N+1]  */
int mzgo_initial_inference(mzgo_engine* eng, const float* obs, int B, float* latent,
                           float* value, float* logits, void* stream);
/*   latent f32 [B][C][N][N], action i64 [B] -> next_latent, reward [B][1], value [B][1], logits */
int mzgo_recurrent_inference(mzgo_engine* eng, const float* latent, const int64_t* action, int B,
                             float* next_latent, float* reward, float* value, float* logits,
                             void* stream);
/* Synchronises ``stream`` and reports (then clears) an out-of-range action seen
 * by mzgo_recurrent_inference (nn.Embedding's IndexError). */
int mzgo_check_inference_errors(mzgo_engine* eng, void* stream);

/* MCTS.run for the first G slots: root_obs f32 [G][6][N][N]; noise f64 [G][A]
 * injected Dirichlet samples or NULL (sampled from the counter RNG keyed by
 * (seed, game_base + g, move_index)).  Outputs: root_child_visits i32 [G][A]
 * (the true child visit counts) and root_value f64 [G] (may be NULL).  The
 * tree stays on the device for mzgo_tree_export. */
int mzgo_search(mzgo_engine* eng, const float* root_obs, const double* noise, int G, int move_index,
                int32_t* root_child_visits, double* root_value, void* stream);
/* Reanalysis (MuZero Reanalyse; no reference counterpart): search n stored
 * positions -- any n >= 1, not bounded by num_games -- under the engine's
 * current weights and search parameters.  All pointers are device pointers.
 * Position i is given in the self-play record format (mzgo_records_export):
 * stones i8 [n][N*N] (0 / 1 black / 2 white), invd u8 [n][N*N], flags u8 [n]
 * (bit0 turn, bit1 passed, bit2 done; bit3: searched with the fast budget,
 * which reanalysis ignores -- it always searches with num_simulations), and
 * ids i32 [n][2] = (key game id, move
 * index): the search's RNG streams are keyed by (seed, ids[i][0], ids[i][1]).
 * The key game id of a self-play record is (game_base + g) ^ (epoch << 24);
 * with it and the record's move index the search is the record's own.  noise
 * f64 [n][A]: injected Dirichlet samples, or NULL (sampled from the counter
 * RNG).  Outputs: visits i32 [n][A], the root's true child visit counts;
 * value f64 [n], the root value; policy f64 [n][A] (may be NULL), the policy
 * target the engine's move rule records under compat "fixed" -- search_variant
 * 0: visits * mask / sum, or mask / sum(mask) when that sum is 0;
 * search_variant 1: counts / sum over the legal actions, and an ALL-ZERO row
 * when no legal child was visited (self-play draws a random action there and
 * records it one-hot; reanalysis draws no action).
 * The call enqueues a memset of the engine's queue-head word and one launch
 * (k_reanalyse_queue) on ``stream``: min(n, CU count, tree slots) persistent
 * workgroups claim items from one queue, each searching in its own tree slot.
 * So the concurrency is bounded by the engine's tree slots (num_games; the CU
 * count on 19x19 compat "reference" engines, see the move-parallel note): an
 * engine made for reanalysis wants num_games >= the CU count.  Afterwards the
 * slot trees belong to whatever items ran last in each slot (the move-parallel
 * note's caveat); boards, records and job slots are untouched, the search
 * counters of mzgo_selfplay_counters ([4], [6]) advance.  Calls on one engine
 * must be ordered (one stream, or synchronised): they share the slots and the
 * queue head.
 * MZGO_EINVAL: null engine or required pointer, n < 1, a board-only engine
 * (latent_dim 0), a tower engine (tower = 1: not supported).  MZGO_ENOWEIGHTS
 * as mzgo_search. */
int mzgo_reanalyse(mzgo_engine* eng, const int8_t* stones, const uint8_t* invd, const uint8_t* flags,
                   const int32_t* ids, const double* noise, int n, int32_t* visits, double* value,
                   double* policy, void* stream);
/* Copy slot g's last search tree to host buffers (synchronises ``stream``):
 * n_nodes; child i32 [n][A]; visits i32 [n]; value_sum f64 [n]; prior f32 [n][A]
 * (row 0 unused); root_prior f64 [A].  Buffers must hold S+1 nodes; NULL skips.
 * After mzgo_search every row is final.  After mzgo_selfplay_move on the
 * reference network (tower = 0), a node that no select reached has NO formed
 * rows: a batched child's policy head is lazy (never computed), so its prior
 * row holds whatever an earlier search left there and its child row either
 * the same stale ids (boards whose tree lives in LDS, 5x5-9x9: the node is
 * marked in the kernel's LDS bitmask) or the sentinel -3 in entry 0 (HBM
 * trees, 19x19); the rows are formed when a select first reaches the node
 * (it has no children before), and the move never reads the others.  Tower
 * engines settle such rows here first (the search API's settle kernel), so
 * their exports are complete. */
int mzgo_tree_export(mzgo_engine* eng, int g, int32_t* n_nodes_host, int32_t* child_host,
                     int32_t* visits_host, double* value_sum_host, float* prior_host,
                     double* root_prior_host, void* stream);

/* GoEnv protocol on the G slots.  board_step: actions i32 [G] (-1 = leave the
 * slot alone); status i32 [G] gets 0 ok, 1 step after done, 2 invalid move,
 * 3 action out of range; winner f64 [G] gets GoEnv.winner() after the step.
 * status/winner may be NULL. */
int mzgo_board_reset(mzgo_engine* eng, void* stream);
int mzgo_board_step(mzgo_engine* eng, const int32_t* actions, int32_t* status, double* winner,
                    void* stream);
/* planes f64 [G][6][N][N] */
int mzgo_board_planes(mzgo_engine* eng, double* planes, void* stream);
/* Overwrite slot g's board (host data): stones i8 [N*N] (0/1 black/2 white),
 * invd u8 [N*N], meta i32 [4] (turn, passed, done, moves). */
int mzgo_board_set(mzgo_engine* eng, int g, const int8_t* stones_host, const uint8_t* invd_host,
                   const int32_t* meta_host, void* stream);

/* Self-play.  selfplay_reset starts a new game in every slot (epoch = RNG
 * generation of the games); selfplay_move plays one move in every unfinished
 * slot.  selfplay_counters (host u64 [8], synchronises; cumulative over the
 * engine's life): [0] simulations run, [1] moves played, [2] games finished,
 * [3] slots still playing now, [4] dynamics 3x3 convs run by searches (one per
 * expansion with direct_dynamics, one per new parent node when factored;
 * tower engines: dynamics towers evaluated, speculative batch entries that
 * were never used included),
 * [5] of those, parent convs shared with the workgroups of games that had
 * already ended (9x9 whole-game launches: the epoch tail), [6] prior rows
 * formed by searches (a node's child priors + child row written to HBM: every
 * eagerly expanded child, and a lazily expanded one -- the lazy policy head --
 * only when a select first reaches it; 0 on tower engines), [7] self-play
 * game workgroups started (every slot's workgroup of every launch counts one
 * when it begins: mzgo_stream_wait_started's count), [8] epoch-tail helper
 * workgroups whose bounded wait for a job expired (they stop helping; records
 * are unaffected).  counters_host must hold 9 values.  An expired
 * mzgo_stream_wait_started gate is reported here (MZGO_EHIP, once). */
int mzgo_selfplay_reset(mzgo_engine* eng, int epoch, void* stream);
int mzgo_selfplay_move(mzgo_engine* eng, void* stream);
/* Up to ``moves`` consecutive moves of every unfinished slot in ONE launch
 * (each slot stops at its game's end); the records and RNG streams are those
 * of ``moves`` mzgo_selfplay_move calls.  moves = max_moves plays whole games.
 * Tower engines (tower = 1) run a move as a sequence of launches; for
 * moves > 4 they read the slots' status every 4 moves (BLOCKING: the stream is
 * synchronised there, so such a call cannot be captured in a HIP graph) and
 * stop enqueueing once every game has ended -- the same records and counters
 * as ``moves`` single-move calls -- and synchronise once at the end of every
 * call, which reports an expired k_tconv_chain wait (MZGO_EHIP). */
int mzgo_selfplay_moves(mzgo_engine* eng, int moves, void* stream);

/* Arena (main.py:526-611, SelfPlayEvaluator): like mzgo_selfplay_move, but
 * game i (global id) is played between two networks -- eng's ("current",
 * turn 0) and opponent's ("best", turn 1); game i's first mover is turn
 * i % 2 and turns alternate.  Search, move rule and records are eng's
 * (use search_variant 1 for main.py's rules); opponent only lends its
 * weights (same board_size and latent_dim).  Replaces the evaluator's
 * MCTS(current/best net).run + argmax loop (main.py:548-568). */
int mzgo_arena_move(mzgo_engine* eng, mzgo_engine* opponent, void* stream);
/* ``moves`` arena moves per slot in one launch (as mzgo_selfplay_moves). */
int mzgo_arena_moves(mzgo_engine* eng, mzgo_engine* opponent, int moves, void* stream);
int mzgo_selfplay_counters(mzgo_engine* eng, uint64_t* counters_host, void* stream);
/* Search statistics of the speculative batches after the root's (boards whose
 * trees live in LDS: 5x5, 6x6, 9x9 with num_simulations + 2 <= 512; zeros
 * elsewhere), summed over every search of the engine since its creation, three
 * values: [0] batch children expanded, [1] batch children whose backup value
 * came from the value cache instead (a batch at the same leaf was cut short
 * before and had computed it; MZGO_VALUE_CACHE=0 at engine creation turns the
 * cache off: [1] stays 0 and [0] counts them), [2] batches cut short by their
 * replay.  Trees and records do not depend on the cache.  Synchronises
 * ``stream``. */
int mzgo_search_stats(mzgo_engine* eng, uint64_t* stats_host, void* stream);
/* The same statistics and those added since, with the room the caller has:
 * writes min(cap, n) values to stats_host, n = 5 today, and nothing past
 * them.  [0..2] as mzgo_search_stats; [3], [4] arrival convs: first arrivals
 * of a select at a lazily expanded node whose parent conv ran at once, the
 * node's priors and the simulation's pick formed under it (9x9 LDS trees with
 * self_play.py's search; MZGO_ARRIVAL_CONV=0 at engine creation keeps the
 * select-then-conv order: both stay 0), split by where the conv and the
 * policy sums read the parent's Y: [3] its LDS copy, [4] L2.  Trees, records
 * and the other counters do not depend on the switch.  Synchronises
 * ``stream``. */
int mzgo_search_stats2(mzgo_engine* eng, uint64_t* stats_host, int cap, void* stream);

/* Move-parallel epoch (no reference counterpart; the schedule, not the
 * protocol): a multi-move mzgo_selfplay_moves under compat "reference"
 * (self_play.py's search) runs as two launches -- k_selfplay_boards, every
 * game's moves without their searches (observation, legal mask, action,
 * policy target, board step, reward: under compat "reference" the action
 * never reads the search), then k_search_queue, which runs every recorded
 * move's search (root value) from one work queue on one workgroup per CU.
 * The records are byte-identical to the game-per-workgroup launch
 * (MZGO_MOVE_PARALLEL=0 in the environment keeps that launch); the trees
 * left in the slots are then those of whatever searches ran last in each
 * queue slot, not one per game.  19x19 engines created under compat
 * "reference" hold a tree slot per CU for it (MZGO_MOVE_PARALLEL=0 at
 * creation: G slots).
 * mzgo_selfplay_set_timing(eng, 1) records HIP events around both launches
 * of every such call (0 stops and discards); mzgo_selfplay_launch_times
 * synchronises on them, writes up to ``cap`` (boards, queue) durations in
 * ms, stores the number recorded in *n_host and clears them. */
int mzgo_selfplay_set_timing(mzgo_engine* eng, int on);
int mzgo_selfplay_launch_times(mzgo_engine* eng, float* boards_ms, float* queue_ms, int cap, int* n_host);
/* DIAGNOSTIC (scripts/rccl_standin.py; not part of the self-play protocol, and
 * bench.py does not call it: it gathers every timed epoch's records in ONE
 * collective after the timed loop).  Enqueue on ``stream`` a gate that
 * completes once counter [7] (self-play workgroups started) reaches
 * ``target``: work queued behind it -- a collective -- cannot take a CU before
 * every workgroup of the self-play launch that brings the count to target is
 * resident (a self-play workgroup fills a CU's LDS).  The gate itself is one
 * wave without LDS, so it sits beside them; its wait is bounded (~seconds)
 * and an expiry is reported by the next mzgo_selfplay_counters call.  Tower
 * engines: MZGO_EINVAL (they never count started workgroups). */
int mzgo_stream_wait_started(mzgo_engine* eng, uint64_t target, void* stream);
/* Tower engines (tower = 1): report (synchronising) and reset the time spent
 * in the dynamics towers since the last call -- one HIP event pair around each
 * simulation step's 2*res_blocks+1 conv launches, on the launch stream -- then
 * switch the timing on (enable = 1) or off. */
int mzgo_tower_timing(mzgo_engine* eng, int enable, double* tower_ms_host, int64_t* towers_host);

/* Trainer backward of the dynamics conv (main.py:478-482's loss.backward()
 * through DynamicsNetwork.forward, main.py:97-103; replaces
 * torch.nn.grad.conv2d_input / conv2d_weight in the trainer's HIP autograd
 * Function).  Forward: out = relu(conv3x3(latent + emb[action]) + bias),
 * padding 1.  In: grad_out, out, latent [B][C][N][N] f32, action [B] i64,
 * emb [A][C], weight [C][C][3][3].  Out: grad_latent [B][C][N][N] (= the
 * conv input's gradient), grad_weight [C][C][3][3], grad_bias [C]; fp32 MFMA,
 * deterministic.  C a multiple of 16, 2 <= N <= 19, 1 <= B <= 65535 (the
 * input gradient's launch has the batch in the grid's z dimension; a larger B
 * is MZGO_EINVAL before any device work); workspace of at least
 * mzgo_dyn_conv_backward_workspace(B, C) bytes (device). */
int mzgo_dyn_conv_backward_workspace(int B, int C, int64_t* bytes_host);
int mzgo_dyn_conv_backward(const float* grad_out, const float* out, const float* latent, const int64_t* action,
                           const float* emb, const float* weight, int B, int C, int N, float* grad_latent,
                           float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                           void* stream);
/* Trainer: one 3x3 conv layer y = relu(conv3x3(x') + bias), padding 1, on
 * fp32 MFMA (main.py:72-84 RepresentationNetwork's conv1-3, main.py:97-103
 * DynamicsNetwork's conv), x' = x [B][Cin][N][N], or x + emb[action[b]]
 * broadcast over the board when emb ([A][Cin]) is given (the dynamics input).
 * Forward: the activation recomputation of the representation's hidden
 * layers (the engine's k_initial_inference keeps them on chip).  Backward:
 * from the saved output (ReLU mask y > 0) and input, grad_x [B][Cin][N][N]
 * (may be NULL: the first layer), grad_weight [Cout][Cin][3][3], grad_bias
 * [Cout]; deterministic (fixed summation order).  Replaces
 * torch.nn.grad.conv2d_input / conv2d_weight in the trainer's autograd
 * Functions.  Any Cin, Cout >= 1; 2 <= N <= 19; 1 <= B <= 65535 (the forward
 * and the input gradient launch a grid with z = B: a larger batch is
 * MZGO_EINVAL, naming the limit, before any device work); device workspace of
 * at least mzgo_conv3x3_backward_workspace(B, Cin, Cout) bytes. */
int mzgo_conv3x3_relu_forward(const float* x, const int64_t* action, const float* emb, const float* weight,
                              const float* bias, int B, int Cin, int Cout, int N, float* out, void* stream);
int mzgo_conv3x3_backward_workspace(int B, int Cin, int Cout, int64_t* bytes_host);
int mzgo_conv3x3_backward(const float* grad_out, const float* out, const float* x, const int64_t* action,
                          const float* emb, const float* weight, int B, int Cin, int Cout, int N, float* grad_x,
                          float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* Test hook: use injected Dirichlet samples f64 [G][max_moves][A] (device,
 * caller-owned, must outlive the moves) instead of the counter-RNG sampler;
 * NULL restores sampling. */
int mzgo_selfplay_inject_noise(mzgo_engine* eng, const double* noise);
/* Test hook (parity of the sampled-noise path): every self-play root's
 * normalised Dirichlet sample -- the one the counter-RNG sampler drew, or the
 * injected one -- written to dst f64 [G][max_moves][A] (device, caller-owned,
 * must outlive the moves) at (slot, move); NULL turns it off. */
int mzgo_selfplay_record_noise(mzgo_engine* eng, double* dst);
/* Test hook, tower engines (tower = 1): every node the searches evaluate,
 * written to dst f32 [G][S+1][A+2] (device, caller-owned) at (slot, node id)
 * as the tower produced it: the policy logits [A], then reward and value
 * (node 0: the representation's logits and value, reward 0).  With it a
 * CPU search driven by these outputs must rebuild the device tree exactly.
 * NULL turns it off. */
int mzgo_tower_record_nodes(mzgo_engine* eng, float* dst);

/* Copy slot g's game record to host buffers (synchronises ``stream``).
 * length: moves recorded; ended: 1 if the game ended by double pass; status.
 * stones i8 [M][N*N], invd u8 [M][N*N], flags u8 [M] (bit0 turn, bit1 passed,
 * bit2 done, bit3: searched with the fast budget -- playout cap randomization,
 * mzgo_config::fast_simulations), action i32 [M], value f64 [M], policy f64 [M][A], reward f64 [M],
 * final_reward f64.  M = length; NULL pointers are skipped. */
int mzgo_records_export(mzgo_engine* eng, int g, int32_t* length_host, int32_t* status_host,
                        int8_t* stones_host, uint8_t* invd_host, uint8_t* flags_host,
                        int32_t* action_host, double* value_host, double* policy_host,
                        double* reward_host, double* final_reward_host, void* stream);

/* All slots' records packed into one DEVICE buffer (the multi-GPU trajectory
 * gather moves it with RCCL).  dst NULL: only report *bytes_needed.  Layout,
 * each field padded to 16 bytes, G slots, M = max_moves, C = N*N, A = C+1:
 *   stones i8 [G][M][C] | invd u8 [G][M][C] | flags u8 [G][M] | action i32 [G][M] |
 *   value f64 [G][M] | policy f64 [G][M][A] | reward f64 [G][M] |
 *   meta i32 [G][4] (turn, passed, done, length) | status i32 [G] | final_reward f64 [G] */
int mzgo_records_pack(mzgo_engine* eng, uint8_t* dst, int64_t capacity, int64_t* bytes_needed,
                      void* stream);

/* Device replay store (no reference counterpart in storage; the semantics are
 * main.py:158-184's PrioritizedReplayBuffer, the targets main.py:381-522's).
 * A FIFO ring of ``capacity`` game slots in HBM, in the self-play record
 * format.  With M = max_moves, C = N*N, A = C + 1 a slot holds
 *   stones i8 [M+1][C], invd u8 [M+1][C], flags u8 [M+1]  the L searched
 *                              positions, then the board after the last move
 *   action i32 [M], policy f64 [M][A], root_value f64 [M]
 *   reward f64 [M+1]           main.py's T+1 rewards, the winner last
 *   length i32, key_gid i32    L, and the game's RNG key id (mzgo_reanalyse's)
 * Logical game i (0 = oldest) lives in slot (head + i) % capacity; a game
 * added to a full store evicts game 0.  The host mirrors only the lengths and
 * key ids (mzgo_replay_info); priorities and sampling are the caller's
 * (mzgo.DeviceReplay keeps main.py's np.random sequence) unless the device
 * ledger and sampler further down are used (mzgo_replay_sample).  Calls on one store
 * must be ordered (one stream, or synchronised): they share index staging and
 * the samplers' working tree.
 * A store is not thread-safe.  Every failure below is reported through
 * mzgo_last_error().
 *
 * mzgo_replay_create: MZGO_EINVAL for a null ``out``, board_size outside
 * 2..19, capacity < 1, max_moves < 1. */
typedef struct mzgo_replay mzgo_replay;
int mzgo_replay_create(int board_size, int capacity, int max_moves, int device, mzgo_replay** out);
void mzgo_replay_destroy(mzgo_replay* replay);
/* Host mirrors: the number of games held, the ring's head slot, and per
 * logical game its length and key id (buffers of ``capacity`` values; any
 * pointer may be NULL).  No device work. */
int mzgo_replay_info(const mzgo_replay* replay, int32_t* size_host, int32_t* head_host, int32_t* lengths_host,
                     int32_t* key_gid_host);
/* Ingest every slot's finished game of ``eng``, device to device, in one
 * launch (k_replay_ingest, a workgroup per game), as G adds in slot order.
 * Reads the records (stones, invd, flags, action, policy, reward, value) up to
 * the game's length (the board's move count, = game_len once the game has
 * ended), the board slot as the final position and final_reward, and applies
 * main.py:699-713's two rules: -0.5 on the last reward when the game hit the
 * move cap without ending; winner = final_reward if the game ended, else 0.
 * key_gid = (game_base + g) ^ (epoch << 24), the record's own search key.
 * The caller makes sure no game is still playing (mzgo_selfplay_counters [3]).
 * Synchronises ``stream`` (the G lengths come back to the host mirror).
 * MZGO_EINVAL: null replay or engine; a board-only engine (latent_dim 0); a
 * tower engine (tower = 1); the engine's board_size or max_moves differs from
 * the store's. */
int mzgo_replay_add_games(mzgo_replay* replay, mzgo_engine* eng, void* stream);
/* Continuous self-play: play ``n_games`` games on the engine's G = num_games
 * slots in ONE launch (k_selfplay_games) and push them into the store as
 * n_games adds in index order.  min(n_games, G, CU count) workgroups each own
 * one engine slot and claim the next game from a device queue when their own
 * ends; a finished game is ingested by the workgroup that played it, under
 * mzgo_replay_add_games' rules.
 *
 * Game j (0 <= j < n_games) IS slot j % G of epoch first_epoch + j / G: its
 * key id is (game_base + j % G) ^ ((first_epoch + j / G) << 24) and every
 * move's RNG key is (seed, that id, move).  The stored games are therefore
 * those of ceil(n_games / G) epochs of mzgo_selfplay_reset(epoch) +
 * mzgo_selfplay_moves(max_moves) + mzgo_replay_add_games (of the last epoch,
 * its first n_games % G games when that is not 0), byte for byte and in that
 * order: game j's ring slot is fixed before the launch, whichever workgroup
 * finishes first.  No helper workgroups and no tail phase run, whatever
 * MZGO_HELPERS_PER_GAME and MZGO_TAIL_HELPERS say; the records do not depend
 * on either.
 *
 * Synchronises ``stream`` once (the n_games lengths and the error word come
 * back to the host mirror) and sets the engine's epoch to first_epoch +
 * ceil(n_games / G) - 1, the last one played.  Counters [0], [1], [2] advance
 * per move and game as in every self-play launch, [7] once per workgroup.
 *
 * THE SLOTS AFTERWARDS: slot b < min(n_games, G, CU count) holds the last
 * game workgroup b played -- games of different epochs, and which game depends
 * on the schedule -- and slots past that are untouched.  mzgo_tree_export,
 * mzgo_records_export, mzgo_records_pack and mzgo_replay_add_games read those
 * slots as they are: the store is this call's result; mzgo_selfplay_reset
 * starts the slots afresh.
 *
 * MZGO_EINVAL: null replay or engine; n_games < 1; n_games > the capacity (a
 * ring slot would be written twice in one launch); a board-only engine; a
 * tower engine; the engine's board_size or max_moves differs from the store's;
 * a noise hook is set (mzgo_selfplay_inject_noise, mzgo_selfplay_record_noise:
 * those buffers are indexed by slot).  Nothing is played or stored then.
 * MZGO_EHIP, after the host mirror is filled: a game stopped on a board error
 * (slot status >= 16); it is stored with the moves it has, the other games are
 * unaffected, and the message names the smallest such j. */
int mzgo_replay_play_games(mzgo_replay* replay, mzgo_engine* eng, int n_games, int first_epoch, void* stream);
/* Add one game from host buffers (synchronises ``stream``): stones i8
 * [L+1][C], invd u8 [L+1][C], flags u8 [L+1], action i32 [L], policy f64
 * [L][A], reward f64 [L+1], root_value f64 [L] (NULL = zeros).  The flags are
 * stored as given (bit0 turn, bit1 passed, bit2 done; bit3: searched with the
 * fast budget -- such a position's t_pol row is all zero in every batch until
 * a reanalysis into the store rewrites the row and clears the bit).
 * MZGO_EINVAL: null replay or required buffer; length outside 0..max_moves. */
int mzgo_replay_add(mzgo_replay* replay, int length, const int8_t* stones_host, const uint8_t* invd_host,
                    const uint8_t* flags_host, const int32_t* action_host, const double* policy_host,
                    const double* reward_host, const double* root_value_host, int32_t key_gid, void* stream);
/* Copy logical game i to host buffers sized for max_moves (the shapes of
 * mzgo_replay_add with L = max_moves; NULL pointers are skipped; synchronises
 * ``stream``).  flags: bit0 turn, bit1 passed, bit2 done, bit3: searched with
 * the fast budget and not reanalysed since (never set on the final board's
 * row L).  MZGO_EINVAL: null replay; i outside 0..size-1. */
int mzgo_replay_export(mzgo_replay* replay, int i, int32_t* length_host, int32_t* key_gid_host, int8_t* stones_host,
                       uint8_t* invd_host, uint8_t* flags_host, int32_t* action_host, double* policy_host,
                       double* reward_host, double* root_value_host, void* stream);
/* The item list of B samples given on the HOST: sample b is logical game
 * indices_host[b] from move starts_host[b] under symmetry symmetries_host[b]
 * (0..7; NULL = identity).  The triples are checked against the host mirror and
 * written as (slot, start, symmetry) through pinned staging words into
 * ``items`` (device i32 [B][3]), the form every assembly below takes and the
 * samplers write: one check and one upload serve any number of assemblies of
 * the same samples.  The call waits until the staging words' previous upload
 * has been read; it does not wait for this one.
 * MZGO_EINVAL: null replay, indices, starts or items; B < 1; an index outside
 * 0..size-1; a start outside 0..L-1 of its game; a symmetry outside 0..7. */
int mzgo_replay_items(mzgo_replay* replay, const int32_t* indices_host, const int32_t* starts_host,
                      const int32_t* symmetries_host, int B, int32_t* items, void* stream);
/* Batch assembly, one launch (k_replay_batch, a workgroup per sample): the
 * trainer's targets (mzgo.trainer batch_targets; main.py:395-470, :503-515)
 * for the B samples of a device item list (i32 [B][3]: slot, start, symmetry,
 * as mzgo_replay_items or a sampler wrote them), with K = unroll_steps, so that
 * a reanalysis of the sampled windows can run between the draw and the
 * assembly.  Device outputs:
 *   obs0 f32 [B][6][N][N]          the observation at ``start``
 *   boot_obs f32 [B][K+1][6][N][N] the observation at start+k+K where the value
 *                                  target of unroll step k has a bootstrap
 *                                  position (start+k+K <= L), zeros elsewhere
 *   acts i64 [B][K]                the actions from ``start``; pass (A-1) past the end
 *   t_rew f32 [B][K]               the rewards from ``start``; 0 past the winner
 *   t_pol f32 [B][K+1][A]          the stored f64 rows rounded to f32;
 *                                  (float)(1.0 / A) past the end; ALL ZERO for a
 *                                  position whose flags carry bit3 (searched with
 *                                  the fast budget: no policy target -- the loss
 *                                  and its gradient are exactly 0 on such a row)
 *   val, factor f64 [B][K+1]       compute_target_value's reward part and the
 *                                  bootstrap's weight: target += factor * r;
 *                                  factor *= discount, in that order in f64,
 *                                  stopping at the rewards' end
 *   has_boot u8 [B][K+1]
 * Symmetry s gives the sample as if its whole trajectory had been transformed:
 * every plane and the first N*N policy entries as [N][N] become np.rot90(x,
 * s & 3), then np.flip(axis=-1) if s & 4; an action below N*N moves where its
 * one-hot would; the pass entry and the pass action stay.
 * The value targets are finished with mzgo_initial_inference over boot_obs's
 * B*(K+1) rows and mzgo_replay_finish_values.
 * The items are not checked against the host mirror, and the kernel reads no
 * row outside the store whatever they hold: a slot outside 0..capacity-1 gives
 * an empty game's outputs (zero planes, pass actions, rewards 0, uniform policy
 * rows, val 0, factor 1, has_boot 0), and so does every row before a game's
 * first.  No host staging, no synchronisation.  MZGO_EINVAL: null replay, items
 * or outputs; B < 1; unroll_steps outside 1..63. */
int mzgo_replay_batch_items(mzgo_replay* replay, const int32_t* items, int B, int unroll_steps, double discount,
                            float* obs0, float* boot_obs, int64_t* acts, float* t_rew, float* t_pol, double* val,
                            double* factor, uint8_t* has_boot, void* stream);
/* t_val[i] = (float)(val[i] + factor[i] * (double)value[i]) where has_boot[i],
 * (float)val[i] elsewhere, for n entries (device pointers; value f32 [n]: the
 * network's values of the boot_obs rows).  MZGO_EINVAL: a null pointer; n < 1. */
int mzgo_replay_finish_values(const double* val, const double* factor, const uint8_t* has_boot, const float* value,
                              int n, float* t_val, void* stream);
/* Reanalysis in place: search the L stored positions of the given logical
 * games (games_host NULL: every game) under ``eng``'s weights and search
 * parameters, position t of a game keyed (key_gid, t), queued latest move
 * first; the fresh policy rows and root values replace the stored ones, and
 * bit3 of every rewritten row's flags is cleared (it is a full-budget target
 * now; mzgo_replay_reanalyse_sample* do the same for the rows they search).  The
 * positions are gathered into staging the store owns, searched by
 * mzgo_reanalyse (whose conditions and errors apply) and scattered back:
 * nothing but the item list (slot, move) crosses the bus.
 * MZGO_EINVAL: null replay or engine; board-size mismatch; a game outside
 * 0..size-1; n_games < 0. */
int mzgo_replay_reanalyse(mzgo_replay* replay, mzgo_engine* eng, const int32_t* games_host, int n_games,
                          void* stream);
/* The index maps k_replay_batch applies for symmetry s on an N x N board
 * (host buffers, no device work): src i32 [N*N], output cell c shows input
 * cell src[c]; dst i32 [N*N+1], action a becomes dst[a] (dst[N*N] = N*N).
 * MZGO_EINVAL: board_size outside 2..19; symmetry outside 0..7. */
int mzgo_replay_symmetry_table(int board_size, int symmetry, int32_t* src_host, int32_t* dst_host);

/* The device priority ledger and sampler (opt-in; independent of whatever
 * priorities the caller keeps on the host).  Per ring slot the store holds a
 * sampling weight prio f64 (already raised to the priority exponent) and a
 * generation gen u32.  mzgo_replay_add_games, mzgo_replay_play_games and
 * mzgo_replay_add give every game they store weight 1.0 and gen + 1 (one small
 * launch on their stream).  A slot whose game has no moves weighs 0.
 *
 * mzgo_replay_sample draws B distinct games by successive sampling without
 * replacement: draw t picks game i with probability w_i / (the sum of the
 * weights not yet picked), from a 64-ary sum tree over the slots (leaves,
 * sums of 64, sums of 64 of those; capacity <= 64^3).  Two launches
 * (k_replay_sample_build: a wave per 64 slots; k_replay_sample_draw: one
 * wave), no host staging, no synchronisation.  With key = stream_key(seed,
 * 0x53414D50, step) (the engine's counter RNG, oracle/rng.py):
 *   u = u01(draw(key, 5, t)); target = u * total; at each of the three levels
 *   the 64 entries' inclusive prefix p comes from six steps d = 1, 2, .., 32 of
 *   p[i] <- (i >= d ? p[i - d] : 0) + p[i]; the pick is the first non-zero
 *   entry with p > target, or the last non-zero entry if rounding left none;
 *   target -= p[pick - 1].  The picked leaf is zeroed and its two ancestors are
 *   summed again (element 63 of the same scan), never subtracted from.
 *   start = randbelow(draw(key, 6, t), length); symmetry = randbelow(draw(key,
 *   7, t), 8) when ``symmetries`` != 0, else 0.
 * Only f64 +, -, x, compares and integer operations decide the choice, so the
 * result is defined bit for bit; mzgo_replay_sample_host is the same functions
 * (csrc/mzgo_replay.hpp) run serially on host arrays in SLOT order.
 * Device outputs: items i32 [B][3] (slot, start, symmetry), index i32 [B]
 * (logical, oldest = 0), gen u32 [B] (the slot's generation at the draw) and,
 * unless NULL, weight f32 [B] = (n_valid w_i / total)^(-beta) over the batch's
 * largest, in f64 pow from the weights before any removal (n_valid = the games
 * with moves).
 * MZGO_EINVAL: null replay, items, index or gen; B < 1; B > the number of
 * stored games with moves (the host mirror's count); capacity > 64^3; beta
 * negative or not finite. */
int mzgo_replay_sample(mzgo_replay* replay, int B, uint64_t seed, uint32_t step, int symmetries, double beta,
                       int32_t* items, int32_t* index, uint32_t* gen, float* weight, void* stream);
/* Reanalysis of a sampled batch's windows, in place and without the host.  A
 * sample (slot, start, symmetry) with K = unroll_steps on a game of L moves
 * reads the stored policy rows t = start .. min(start + K, L - 1) (rows past
 * the end are the uniform row and are not stored): its window.  A triple whose
 * slot is outside 0..capacity-1, whose game has L <= 0 or whose start is
 * outside 0..L-1 has none.  The call enqueues, in order: k_replay_window_items
 * (one workgroup, no atomics) writing every (slot, t) of every window by
 * falling t, equal t by batch position, and their count n into memory the
 * store owns (and n into *n_searched unless NULL); a memset of the engine's
 * queue head; and the in-place reanalysis queue on min(B (K + 1), CUs, tree
 * slots) workgroups, which searches exactly those n positions under ``eng``'s
 * weights and search parameters -- position t of a game keyed (seed, key_gid,
 * t), as mzgo_replay_reanalyse keys it -- reading each position from the
 * store's rows and writing the visit-count policy row and the root value into
 * the store's.  Rows outside the windows, and every other field, stay as they
 * are.  No index, position or policy crosses the bus; no synchronisation
 * (after the first call of a size, which allocates the list).  Calls on one
 * store or engine must be ordered.
 * MZGO_EINVAL: null replay, engine or items; B < 1; unroll_steps outside
 * 1..63; board-size mismatch; a board-only engine; a tower engine.
 * MZGO_ENOWEIGHTS as mzgo_search. */
int mzgo_replay_reanalyse_sample(mzgo_replay* replay, mzgo_engine* eng, const int32_t* items, int B,
                                 int unroll_steps, int32_t* n_searched, void* stream);
/* The window rule's host twin (no device work; csrc/mzgo_replay.hpp's functions
 * run serially): length i32 [cap] in slot order, items i32 [B][3]; out i32
 * [B (K + 1)][2] receives the (slot, t) list in the order above and *n its
 * length.  MZGO_EINVAL: a null pointer; cap < 1; B < 1; unroll_steps outside
 * 1..63. */
int mzgo_replay_window_items_host(const int32_t* length, int cap, const int32_t* items, int B, int unroll_steps,
                                  int32_t* out, int32_t* n);
/* Search-value targets (opt-in): value targets from the root values the
 * searches left in the store, without a bootstrap inference.  A game has L
 * moves, rewards r[0..L] (r[L] the winner entry) and root values nu[0..L-1];
 * the target of trajectory index i >= 0 with step horizon n = td_steps >= 1 is
 *   target = 0.0; factor = 1.0                                          (f64)
 *   for j = i .. i + n - 1:  if j > L: break
 *                            target += factor * r[j]; factor *= discount  (in this order)
 *   if      i + n <= L - 1:  target += factor * nu[i + n]
 *   else if i + n == L:      target += factor * r[L]
 *   t_val = (float)target
 * with no contraction, so the result is defined bit for bit (the rule is one
 * function, search_value_target in csrc/mzgo_replay.hpp, which the kernel and
 * the host twin both run).  The i + n == L case is deliberate: the final board
 * is never searched, so nothing is stored for it, and r[L] is the exact
 * remainder of the return from there; network targets (mzgo_replay_batch_items)
 * evaluate the final board at that index instead, so the two kinds of target
 * differ there even when nu holds the network's values.  td_steps is
 * independent of unroll_steps.
 *
 * mzgo_replay_batch_items_values is mzgo_replay_batch_items with one launch of
 * k_replay_batch<true>: obs0, acts, t_rew and t_pol as that writes them (the
 * same symmetry gather), and t_val f32 [B][K+1], entry k the target of index
 * start + k (0 where mzgo_replay_batch_items gives an empty game's outputs); no
 * boot_obs, val, factor or has_boot, and nothing to finish.  The same promises
 * on staging and synchronisation.  MZGO_EINVAL as mzgo_replay_batch_items (for
 * the five outputs it takes), plus td_steps < 1. */
int mzgo_replay_batch_items_values(mzgo_replay* replay, const int32_t* items, int B, int unroll_steps, int td_steps,
                                   double discount, float* obs0, int64_t* acts, float* t_rew, float* t_pol,
                                   float* t_val, void* stream);
/* mzgo_replay_reanalyse_sample over every stored row a search-value batch
 * reads: a sample's window t = start .. min(start + K, L - 1) (its policy
 * rows) together with its value rows t = start + n .. min(start + K + n, L - 1),
 * n = td_steps, each row once per sample (for n > K + 1 a gap lies between the
 * two ranges; a sample with start + n > L - 1 has no value rows).  The same
 * order (falling t, equal t by batch position), launches, queue and promises;
 * the list memory the store owns holds 2 B (K + 1) pairs for this call, and
 * the queue runs on min(2 B (K + 1), CUs, tree slots) workgroups.
 * MZGO_EINVAL and MZGO_ENOWEIGHTS as mzgo_replay_reanalyse_sample, plus
 * td_steps < 1. */
int mzgo_replay_reanalyse_sample_values(mzgo_replay* replay, mzgo_engine* eng, const int32_t* items, int B,
                                        int unroll_steps, int td_steps, int32_t* n_searched, void* stream);
/* The target rule's host twin (no device work): reward f64 [L + 1], root_value
 * f64 [L] (may be NULL when L = 0); t_val f32 [unroll_steps + 1] receives the
 * targets of indices start .. start + unroll_steps.  MZGO_EINVAL: a null
 * pointer; L outside 0..2^30; start < 0; unroll_steps outside 1..63;
 * td_steps < 1. */
int mzgo_replay_value_targets_host(const double* reward, const double* root_value, int L, int start, int unroll_steps,
                                   int td_steps, double discount, float* t_val);
/* The host twin of mzgo_replay_reanalyse_sample_values' item list (no device
 * work): as mzgo_replay_window_items_host, with out i32 [2 B (K + 1)][2].
 * MZGO_EINVAL as there, plus td_steps < 1. */
int mzgo_replay_window_items_values_host(const int32_t* length, int cap, const int32_t* items, int B, int unroll_steps,
                                         int td_steps, int32_t* out, int32_t* n);
/* The sampler's host twin (no device work): prio f64 [cap] and length i32
 * [cap] in slot order, ``head`` the slot of logical game 0; host outputs
 * items, index and (unless NULL) weight as above.  MZGO_EINVAL: a null
 * pointer; cap outside 1..64^3; head outside 0..cap-1; B < 1 or > the slots
 * with length > 0; a weight of such a slot that is not finite and > 0; beta. */
int mzgo_replay_sample_host(const double* prio, const int32_t* length, int cap, int head, int B, uint64_t seed,
                            uint32_t step, int symmetries, double beta, int32_t* items, int32_t* index,
                            float* weight);
/* New weights for a sampled batch (k_replay_update_priorities, a thread per
 * sample; device pointers; does not synchronise).  Slot items[b][0] gets
 * pow(max(p, FLT_MIN), alpha) -- exactly max(p, FLT_MIN) at alpha == 1 -- with
 * p = per[b] (f32, a loss per sample) or *mean (f64, one value for all B);
 * exactly one of the two is non-NULL.  A slot whose generation no longer
 * equals gen[b] (a newer game has taken it) keeps its weight; so does a slot
 * whose p is NaN, infinite or negative, and those are counted
 * (mzgo_replay_skipped_updates).  MZGO_EINVAL: null replay, items or gen; B <
 * 1; per and mean both or neither; alpha not finite or <= 0. */
int mzgo_replay_update_priorities(mzgo_replay* replay, const int32_t* items, const uint32_t* gen, const float* per,
                                  const double* mean, int B, double alpha, void* stream);
/* The weights and generations of the games held, in logical order, copied to
 * device buffers of ``size`` entries (either may be NULL; no synchronisation). */
int mzgo_replay_priorities(mzgo_replay* replay, double* prio, uint32_t* gen, void* stream);
/* Set the weights of the n = size games held from a host buffer in logical
 * order (synchronises).  MZGO_EINVAL: n != size; a value not finite and > 0. */
int mzgo_replay_set_priorities(mzgo_replay* replay, const double* values_host, int n, void* stream);
/* The number of priority updates refused so far (synchronises). */
int mzgo_replay_skipped_updates(mzgo_replay* replay, int64_t* count_host, void* stream);

/* Position-level prioritized replay (opt-in on top of the ledger above; MuZero,
 * App. G): a sampling weight per stored POSITION, pprio f64 [capacity][max_moves]
 * (already raised to alpha; rows t >= the game's length are never read), and a
 * sampler that draws (game, start) with probability w[game][start] / total.
 * Nothing is allocated until mzgo_replay_enable_positions (pprio and the
 * counts of positions; the sampler's working tree is the store's one, which
 * mzgo_replay_sample draws from as well); until then every
 * device call below returns MZGO_EINVAL and mzgo_last_error() names it.
 *
 * The weight of a position whose value error is err is
 *   pow(max(err, floor), alpha)   -- exactly max(err, floor) at alpha == 1
 * with floor > 0 (0 selects FLT_MIN, the floor of mzgo_replay_update_priorities;
 * a caller may raise it so that no position starves).  A new game (stored by
 * mzgo_replay_add_games, _play_games or _add: one more small launch on their
 * stream, k_replay_new_positions, next to the one that sets weight 1.0 and
 * gen + 1; the games held at the time of the enabling call get the same) has
 *   init_mode 0 (td):      err_t = |nu[t] - (double)target(t)|, target the
 *                          search-value target of index t with n = td_steps
 *                          under ``discount`` (above; the same function)
 *   init_mode 1 (uniform): weight 1.0 for every position.
 * MZGO_EINVAL: null replay; max_moves > 4096 (two levels of 64 inside a game);
 * capacity > 64^3; td_steps < 1; discount not finite; alpha not finite or <= 0;
 * floor negative or not finite; init_mode; a second call with other parameters
 * (one with the same is a no-op). */
int mzgo_replay_enable_positions(mzgo_replay* replay, int td_steps, double discount, double alpha, double floor,
                                 int init_mode, void* stream);
/* mzgo_replay_sample over positions.  A game's weight is not stored; it is the
 * sum of its positions' weights in the sampler's one order of additions: rows
 * 0..L-1 in chunks of 64, a chunk's sum element 63 of the six-step scan, the
 * game's weight element 63 of the scan over its <= 64 chunk sums, entries past
 * the end 0.  k_replay_possample_build (a workgroup per 64 slots) writes the
 * leaves (that weight, 0 for a game without moves), the sums of 64 leaves and
 * the count of stored positions n_pos; k_replay_possample_draw (one wave)
 * descends the same three levels with the same u, rules and fallback, then
 * carries the remainder of the same target through two more levels of the same
 * rule -- the picked game's chunk sums (formed again, the same additions, so
 * the same bits), then the picked chunk's 64 positions: start is the picked
 * position (tag 6 is not drawn).  The picked game's leaf is zeroed and its
 * ancestors summed again, so the B games are distinct; symmetry, index and gen
 * as mzgo_replay_sample; weight f32 [B] = (n_pos w / total)^(-beta) over the
 * batch's largest, w the picked position's weight, total the sum before any
 * removal.  The items feed mzgo_replay_batch_items, _batch_items_values and
 * mzgo_replay_reanalyse_sample(_values) unchanged.  MZGO_EINVAL as
 * mzgo_replay_sample. */
int mzgo_replay_sample_positions(mzgo_replay* replay, int B, uint64_t seed, uint32_t step, int symmetries,
                                 double beta, int32_t* items, int32_t* index, uint32_t* gen, float* weight,
                                 void* stream);
/* New weights for a sampled batch's windows (k_replay_update_position_priorities,
 * a thread per (sample b, unroll step k); device pointers; no synchronisation):
 * position t = items[b][1] + k of slot items[b][0] gets the weight of err =
 * |(double)value[b][k] - (double)t_val[b][k]|, value and t_val f32 [B][K + 1]:
 * the RAW value head outputs and the RAW value targets (a value transform
 * shapes the loss, not the priority).  Left alone: a slot whose generation no
 * longer equals gen[b], rows t >= the game's length, and an err that is NaN or
 * infinite, which is counted (mzgo_replay_skipped_updates).  MZGO_EINVAL: null
 * pointers; B < 1; unroll_steps outside 1..63. */
int mzgo_replay_update_position_priorities(mzgo_replay* replay, const int32_t* items, const uint32_t* gen,
                                           const float* value, const float* t_val, int B, int unroll_steps,
                                           void* stream);
/* The position weights of the games held, in logical order (oldest first),
 * copied to a device buffer f64 [size][max_moves] (rows t >= a game's length
 * are unspecified; no synchronisation). */
int mzgo_replay_position_priorities(mzgo_replay* replay, double* pprio, void* stream);
/* Set them from a host buffer f64 [n = size][max_moves] in logical order (a test
 * hook; synchronises).  MZGO_EINVAL: n != size; an entry t < length that is
 * negative or not finite; a game with moves whose entries are all 0 (single
 * zeros are allowed). */
int mzgo_replay_set_position_priorities(mzgo_replay* replay, const double* values_host, int n, void* stream);
/* The position sampler's host twin (no device work): pprio f64 [cap][M] and
 * length i32 [cap] in slot order; outputs as mzgo_replay_sample_host.
 * MZGO_EINVAL as there, plus M outside 1..4096, an entry t < length that is
 * negative or not finite, and a game with moves whose weight is not finite
 * and > 0. */
int mzgo_replay_sample_positions_host(const double* pprio, const int32_t* length, int cap, int M, int head, int B,
                                      uint64_t seed, uint32_t step, int symmetries, double beta, int32_t* items,
                                      int32_t* index, float* weight);
/* The td rule's host twin (no device work): reward f64 [L + 1], root_value f64
 * [L]; pprio f64 [L] receives the new-game weights.  floor 0 = FLT_MIN.
 * MZGO_EINVAL: a null pointer; L outside 0..4096; td_steps < 1; alpha; floor. */
int mzgo_replay_position_priorities_host(const double* reward, const double* root_value, int L, int td_steps,
                                         double discount, double alpha, double floor, double* pprio);

/* --------------------------------------------------------------------------
 * The trainer's unroll loss in one launch (main.py:431-482: the value, policy
 * and reward losses of a trajectory's K + 1 unroll steps, which the reference
 * and mzgo.trainer's batched step build from log_softmax, kl_div, two value
 * transforms, two mse_loss and their weights and sums, step by step; this call
 * replaces that protocol and its autograd graph for B samples at once).
 * All pointers are device pointers to contiguous f32 unless said otherwise.
 *   logits [K+1][B][A], value [K+1][B], reward [K][B]   the heads' outputs,
 *                              step-major (the unroll's outputs stacked)
 *   t_pol [B][K+1][A], t_val [B][K+1], t_rew [B][K]     the targets,
 *                              sample-major (mzgo_replay_batch_items' layout)
 * Per row (b, k), with m = max_a logits, s = sum_a exp(logits - m),
 * logp = logits - m - log s, p = exp(logits - m) / s and T = sum_a t_pol:
 *   policy  w_policy * sum_a (xlogy(t, t) - t logp_a); an entry t == 0 adds
 *           exactly 0 (F.kl_div); d/d logits_a = w_policy (p_a T - t_a), with
 *           the row's own T (the (float)(1.0 / A) rows do not sum to 1)
 *   value   w_value d^2, d = h(v) - h(t) with h(x) = sign(x)(sqrt(|x| + 1) - 1)
 *           + 0.001 x (main.py:66-69) when value_transform != 0, else v - t;
 *           d/dv = w_value 2 d h'(v), h'(v) = 0.5 / sqrt(|v| + 1) + 0.001 for
 *           v != 0 and 0.001 at v == 0 (autograd's value: sign(0) = 0)
 *   reward  (k >= 1) w_reward (r - t)^2; d/dr = w_reward 2 (r - t)
 * Outputs:
 *   per_sample f32 [B]   a sample's terms summed in k order: (value + policy)
 *                        of row 0, then + reward + value + policy per row
 *   totals f64 [4]       loss, value part, policy part, reward part over all
 *                        samples, from a fixed-order f64 reduction
 *   g_logits, g_value, g_reward   d (sum_b per_sample[b]) / d input, in the
 *                        inputs' layouts
 * Two launches (k_unroll_loss: a workgroup per sample, a wave per row;
 * k_unroll_loss_totals: one workgroup), no atomics: the same inputs give the
 * same bits.  Does not synchronise.  The per-sample parts pass between the
 * launches in a buffer the library keeps per device, so calls on one device
 * must be ordered (one stream, or synchronised); it grows (synchronising
 * ``stream``) only when B exceeds 4096 and every earlier B.
 * K == 0 has no reward tensors: reward, t_rew and g_reward may be NULL.
 * MZGO_EINVAL, with the reason in mzgo_last_error(): B < 1; K < 0; A outside
 * 2..362; a null required pointer. */
int mzgo_unroll_loss(const float* logits, const float* value, const float* reward, const float* t_pol,
                     const float* t_val, const float* t_rew, int B, int K, int A, float w_value, float w_policy,
                     float w_reward, int value_transform, float* per_sample, double* totals, float* g_logits,
                     float* g_value, float* g_reward, void* stream);
/* The host twin: the same scalar functions (csrc/mzgo_loss.hpp) run serially
 * over HOST arrays of the same layouts; the sums over a row run in entry
 * order.  No device work.  The same MZGO_EINVAL conditions. */
int mzgo_unroll_loss_host(const float* logits, const float* value, const float* reward, const float* t_pol,
                          const float* t_val, const float* t_rew, int B, int K, int A, float w_value, float w_policy,
                          float w_reward, int value_transform, float* per_sample, double* totals, float* g_logits,
                          float* g_value, float* g_reward);

/* --------------------------------------------------------------------------
 * The trainer's whole unroll in one forward and one backward call
 * (main.py:431-482 unrolls a trajectory step by step through
 * RepresentationNetwork, main.py:72-84, K times DynamicsNetwork,
 * main.py:97-113, and PredictionNetwork, main.py:116-144, on every latent;
 * these calls replace that protocol and its autograd graph for B samples at
 * once: the 3 + K convs in sequence on the fp32 MFMA kernels of
 * mzgo_conv3x3_relu_forward / mzgo_conv3x3_backward, the heads of all K + 1
 * latents in one launch each way).  fp32, deterministic (fixed summation
 * orders, no atomics: the same inputs give the same bits), everything
 * enqueued on ``stream``; no call allocates or synchronises.
 *
 * Parameters and gradients are key / pointer tables in the convention of
 * mzgo_set_weights_device: ``keys`` names each of the 22 reference state_dict
 * tensors once, in any order; ``params[i]`` is the tensor (device f32,
 * contiguous) with ``shapes[i]`` / ``ndims[i]`` its state_dict shape for
 * latent_dim C -- the embedding [emb_rows][C] with emb_rows >= N*N + 1 (a
 * table larger than the board, play.py:193, is taken whole); ``grads[i]``
 * (backward) receives the gradient of ``keys[i]``, same shape.
 *
 * mzgo_unroll_workspace: the sizes of the two caller-owned device buffers,
 * ``saved`` (written by the forward, read by the backward: the observations,
 * the representation's two hidden activations, the K + 1 latents
 * [K+1][B][C][N][N] step-major, the heads' two board means per (step, sample)
 * and the actions step-major) and ``work`` (the backward's scratch: the
 * latents' gradients, the conv weight partials, the heads' partial sums).
 *
 * mzgo_unroll_forward: obs0 [B][6][N][N], acts i64 [B][K] (the action taken
 * before step k, sample-major as mzgo_replay_batch_items returns them; values
 * 0 <= a < emb_rows are the caller's contract, as in mzgo_dyn_conv_backward).
 *   latent_0 = representation(obs0); latent_k = relu(conv(latent_{k-1} +
 *   emb[acts[:, k-1]]) + bias)
 *   logits [K+1][B][A], A = N*N + 1: policy_conv (C -> 1) per cell, the pass
 *                       logit in column A - 1
 *   value [K+1][B]      value_fc(mean over the board of value_conv(latent))
 *   reward [K][B]       row k - 1, for steps k >= 1: fc_reward_output(relu(
 *                       fc_reward_hidden(mean of reward_conv(latent_k))))
 * in mzgo_unroll_loss's step-major layouts.  K + 5 launches.  K == 0 is legal:
 * acts and reward may be NULL.
 *
 * mzgo_unroll_backward: from ``saved`` and the gradients with respect to the
 * three outputs (same layouts; g_reward may be NULL at K == 0), the gradients
 * of all 22 parameters; there is no input gradient.
 *   (a) one launch gives every latent's gradient from its heads,
 *       G[s][b][c][p] = w_pol[c] g_logits[s,b,p] + (w_val[c] dvmean[s,b] +
 *       w_rew[c] drmean[s,b]) / N^2, and a row of partial sums per (step,
 *       sample) for the thirteen head tensors (the weights and biases of
 *       policy_conv, value_conv, value_fc, reward_conv, fc_reward_hidden and
 *       fc_reward_output, and pass_logit); a second sums the rows in a fixed
 *       order.  A hidden reward unit whose pre-activation is <= 0 passes
 *       nothing back (autograd's relu).
 *   (b) for s = K .. 1 the dynamics conv's input gradient from G[s] masked by
 *       latent_s > 0 is added into G[s-1]; its board sums are kept.
 *   (c) the dynamics conv's weight and bias gradients in ONE pass over the
 *       K B boards (steps 0..K-1 the inputs, 1..K the outputs and masks):
 *       mzgo_conv3x3_backward's chunked fixed-order sum, with 8 boards per
 *       chunk, or the next multiple of 8 that keeps the partials within 32 MiB
 *       (at most one chunk of all K B boards, whatever that takes: from
 *       C = 976 a single chunk's C*C*36 bytes exceed it).
 *   (d) the embedding gradient [emb_rows][C]: a row is the sum, in (step,
 *       sample) order, of the board sums whose action it is; every other row
 *       is 0 (nn.Embedding's dense gradient).
 *   (e) the representation's three layers from the saved activations.
 * K + 17 launches.  At K == 0 the nine dynamics gradients (embedding, conv,
 * reward_conv, fc_reward_hidden, fc_reward_output) are not written and their
 * ``grads`` entries may be NULL.
 *
 * MZGO_EINVAL, with the reason in mzgo_last_error(), before any device work:
 * B < 1; K < 0; C not a multiple of 16; N outside 2..19; emb_rows < N*N + 1;
 * (K + 1) B above 2^31 - 1; B above 65535 (the convs and the chain launch a
 * grid with z = B); a null required pointer; a missing, duplicate or unexpected key or a shape
 * that is not the state_dict's; saved_bytes / work_bytes smaller than
 * mzgo_unroll_workspace reports. */
int mzgo_unroll_workspace(int B, int K, int C, int N, int emb_rows, int64_t* saved_bytes, int64_t* work_bytes);
int mzgo_unroll_forward(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                        const int* ndims, int n_params, const float* obs0, const int64_t* acts, int B, int K, int C,
                        int N, int emb_rows, void* saved, int64_t saved_bytes, float* logits, float* value,
                        float* reward, void* stream);
int mzgo_unroll_backward(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                         const int* ndims, float* const* grads, int n_params, const void* saved, int64_t saved_bytes,
                         const float* g_logits, const float* g_value, const float* g_reward, int B, int K, int C, int N,
                         int emb_rows, void* work, int64_t work_bytes, void* stream);

/* --------------------------------------------------------------------------
 * bf16 mixed precision for the dynamics conv (csrc/mzgo_conv_bf16.hip).
 *
 * With R(t) = float32 -> bfloat16 round-to-nearest-even, returned as float32
 * (torch's t.bfloat16().float(): NaN stays NaN, overflow goes to inf), the
 * mode changes the dynamics conv's three matrix products only:
 *   forward          y  = relu(conv3x3(R(x + emb[a]), R(W)) + b)
 *   input gradient   gx = conv3x3^T(R(gp), R(W)),  gp = g [y > 0]
 *   weight gradient  gw = corr(R(gp), R(x + emb[a]))
 * on v_mfma_f32_16x16x32_bf16: exact products, float32 accumulation in a
 * fixed order (no atomics: repeats give the same bits).  The add x + emb[a],
 * the bias, the ReLU, every stored tensor, the bias gradient (the float32 sum
 * of the unrounded gp) and the weights themselves stay float32; rounding is
 * straight-through.  Cin and Cout must be multiples of 32 (the MFMA's K) and
 * 2 <= N <= 19: anything else is MZGO_EINVAL, naming the value, before any
 * launch.
 *
 * mzgo_bf16_round_host: out[i] = R(in[i]) on host arrays, compiled from the
 * function the kernels round with.
 *
 * mzgo_conv3x3_relu_forward_bf16 / mzgo_conv3x3_backward_bf16_workspace /
 * mzgo_conv3x3_backward_bf16: one layer, with the arguments of
 * mzgo_conv3x3_relu_forward / _backward_workspace / _backward.  ``weight`` is
 * the float32 tensor [Cout][Cin][3][3]: the forward rounds it while staging,
 * the backward packs R(weight) into its workspace (16-byte aligned), which is
 * mzgo_conv3x3_backward_workspace(B, Cin, Cout) rounded up to 256, plus
 * 36 Cin Cout bytes for the two packed layouts ([tap][co][ci] and
 * [tap][ci][co], bf16).  grad_x may be NULL.
 *
 * mzgo_unroll_workspace_p / _forward_p / _backward_p: the three unroll calls
 * with ``precision``.  MZGO_PREC_F32 is mzgo_unroll_workspace / _forward /
 * _backward exactly (those are calls of these).  MZGO_PREC_BF16 runs the K
 * dynamics convs, the K chain steps and the weight pass in the mode above:
 * the forward packs R(dynamics.conv.weight) once into ``saved``, which grows
 * by 36 C C bytes (rounded up to 256), and the backward reads it there, so the
 * weights must not change between the two calls; ``work`` keeps its size and
 * the weight pass its chunks.  C must be a multiple of 32.  At K == 0 the mode
 * changes nothing, and at K >= 1 logits[0] and value[0] are the float32
 * mode's bits.  The backward must be given the forward's precision. */
enum { MZGO_PREC_F32 = 0, MZGO_PREC_BF16 = 1 };
int mzgo_bf16_round_host(const float* in, int64_t n, float* out);
int mzgo_conv3x3_relu_forward_bf16(const float* x, const int64_t* action, const float* emb, const float* weight,
                                   const float* bias, int B, int Cin, int Cout, int N, float* out, void* stream);
int mzgo_conv3x3_backward_bf16_workspace(int B, int Cin, int Cout, int64_t* bytes_host);
int mzgo_conv3x3_backward_bf16(const float* grad_out, const float* out, const float* x, const int64_t* action,
                               const float* emb, const float* weight, int B, int Cin, int Cout, int N, float* grad_x,
                               float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                               void* stream);
int mzgo_unroll_workspace_p(int B, int K, int C, int N, int emb_rows, int precision, int64_t* saved_bytes,
                            int64_t* work_bytes);
int mzgo_unroll_forward_p(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                          const int* ndims, int n_params, const float* obs0, const int64_t* acts, int B, int K, int C,
                          int N, int emb_rows, void* saved, int64_t saved_bytes, float* logits, float* value,
                          float* reward, int precision, void* stream);
int mzgo_unroll_backward_p(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const void* saved,
                           int64_t saved_bytes, const float* g_logits, const float* g_value, const float* g_reward,
                           int B, int K, int C, int N, int emb_rows, void* work, int64_t work_bytes, int precision,
                           void* stream);

/* The heads' host twin: the same scalar functions (csrc/mzgo_unroll.hpp) run
 * serially over HOST arrays -- forward and backward of the heads of S = K + 1
 * steps' latents [S][B][C][N][N] (every channel and cell sum in index order).
 * The tables hold the thirteen head tensors only; ``grads`` receives their
 * gradients and g_latent [S][B][C][N][N] the latents' (step (a) above).  At
 * S == 1 reward, g_reward and the reward head's ``grads`` may be NULL.  No
 * device work.  MZGO_EINVAL as above (S < 1 for K < 0). */
int mzgo_unroll_heads_host(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const float* latents, int S, int B,
                           int C, int N, float* logits, float* value, float* reward, const float* g_logits,
                           const float* g_value, const float* g_reward, float* g_latent);

/* The unroll's latents, for an auxiliary loss on them.
 *
 * mzgo_unroll_latents: where the latents of a forward call lie inside its
 * ``saved`` buffer -- *bytes = (K + 1) B C N N floats from byte *offset_bytes
 * (a multiple of 256), step-major [K+1][B][C][N][N], float32 in both
 * precisions -- so that a caller can read them in place.  They are the
 * backward's saved activations: they must not be written.
 *
 * mzgo_unroll_backward_l: mzgo_unroll_backward_p with ``g_latent``, the
 * caller's gradient with respect to those latents, laid out like them and
 * 16-byte aligned (``work`` too), or NULL.  When given it is added to the
 * heads' latent gradient after step (a) and before the chain by one elementwise
 * launch (a thread per four floats; float32 in both precisions): the latents
 * are post-ReLU, and the chain and the representation mask with the saved
 * latents, so nothing else changes.  With NULL the launches and every bit are
 * mzgo_unroll_backward_p's (which is this call with NULL).  The same
 * MZGO_EINVAL conditions, and a misaligned g_latent. */
int mzgo_unroll_latents(int B, int K, int C, int N, int emb_rows, int precision, int64_t* offset_bytes,
                        int64_t* bytes);
int mzgo_unroll_backward_l(const char* const* keys, const float* const* params, const int64_t* const* shapes,
                           const int* ndims, float* const* grads, int n_params, const void* saved,
                           int64_t saved_bytes, const float* g_logits, const float* g_value, const float* g_reward,
                           const float* g_latent, int B, int K, int C, int N, int emb_rows, void* work,
                           int64_t work_bytes, int precision, void* stream);

/* --------------------------------------------------------------------------
 * The ownership auxiliary target (KataGo's ownership head on MuZero's unrolled
 * latents; not in main.py): a 1x1 conv C -> 1 on every latent predicts, per
 * board point, who owns it on the game's final board, from the side of the
 * colour to move at that unroll step.
 *
 * Targets.  On the stored final board (row L of a game: 1 black, 2 white, 0
 * empty) a stone is owned by its colour, an empty point by the one colour its
 * empty region touches, by nobody when the region touches both colours or none
 * (oracle/gogame.py: areas, cell by cell).  For sample (slot, start, symmetry)
 * and unroll step k, with at = start + k and mover = 1 + (flags[at] & 1):
 *   t_own [B][K+1][N*N]  +1 where the owner of cell sym_src(N, sym, c) is the
 *                        mover, -1 where it is the other colour, 0 for nobody
 *   own_mask [B][K+1]    1 if at <= L and the game ended (the done bit, bit 2,
 *                        of row L's flags: the condition under which reward[L]
 *                        is the winner), else 0 with an all-zero row -- a game
 *                        cut off by the move cap has no ownership target
 * mzgo_replay_ownership_items takes DEVICE items [B][3] (mzgo_replay_items' or
 * a sampler's): nothing crosses the bus and nothing synchronises.  One launch,
 * a workgroup per sample, next to the batch assembly.  unroll_steps in
 * 0..63.  mzgo_ownership_host is the owner map alone on HOST arrays (stones
 * int8 [N*N] -> owner int8 [N*N]: 0, 1, 2) and mzgo_ownership_targets_host one
 * sample's rows from the final board's stones and the game's flags [L + 1]:
 * the kernel's own functions (csrc/mzgo_replay.hpp), no device work. */
int mzgo_replay_ownership_items(mzgo_replay* replay, const int32_t* items, int B, int unroll_steps, float* t_own,
                                float* own_mask, void* stream);
int mzgo_ownership_host(const int8_t* stones, int board_size, int8_t* owner);
int mzgo_ownership_targets_host(const int8_t* final_stones, const uint8_t* flags, int L, int board_size, int start,
                                int symmetry, int unroll_steps, float* t_own, float* own_mask);

/* The head and its loss on ``latents`` [K+1][B][C][N][N] (mzgo_unroll_latents'
 * layout), head weight w [C] and bias [1]:
 *   x[s][b][c]  = sum_ch w[ch] latents[s][b][ch][c] + bias        (f64 sum, rounded to float32)
 *   l(x, t)     = softplus(2 x) - (1 + t) x,  softplus(z) = max(z, 0) + log1p(exp(-|z|))
 *                 (the cross entropy of (1 + tanh x) / 2 against (1 + t) / 2; d l / d x = tanh(x) - t)
 *   per[b]      = weight sum_k own_mask[b][k] (1 / N^2) sum_c l(x[k][b][c], t_own[b][k][c])
 * mzgo_ownership_loss writes per f32 [B], *total (f64, the samples' sums) and
 * g_x f32 [K+1][B][N*N], the derivative of sum_b per[b] with respect to x:
 * two launches.  mzgo_ownership_loss_backward takes the incoming g_per [B] and
 * writes g_latents[s][b][ch][c] = g_per[b] w[ch] g_x[s][b][c], g_w [C] and
 * g_bias [1]: two launches.  Both use the caller-owned ``work``
 * (mzgo_ownership_loss_workspace bytes: the rows' losses, then the rows'
 * partial sums), which the pair may share; all sums are f64 in a fixed order,
 * no atomics, so repeats are bit-identical.  A row whose mask is 0 is not read
 * and contributes an exact 0 to the loss and to every gradient.  All pointers
 * are device pointers; nothing allocates or synchronises.
 * mzgo_ownership_loss_host is both on HOST arrays with serial sums in index
 * order (csrc/mzgo_ownership.hpp's functions): no device work.  MZGO_EINVAL: a
 * null pointer, B < 1, K < 0, C < 1, N outside 2..19, work too small. */
int mzgo_ownership_loss_workspace(int B, int K, int C, int64_t* work_bytes);
int mzgo_ownership_loss(const float* latents, const float* w, const float* bias, const float* t_own,
                        const float* own_mask, int B, int K, int C, int N, float weight, float* per, double* total,
                        float* g_x, void* work, int64_t work_bytes, void* stream);
int mzgo_ownership_loss_backward(const float* latents, const float* w, const float* own_mask, const float* g_x,
                                 const float* g_per, int B, int K, int C, int N, float* g_latents, float* g_w,
                                 float* g_bias, void* work, int64_t work_bytes, void* stream);
int mzgo_ownership_loss_host(const float* latents, const float* w, const float* bias, const float* t_own,
                             const float* own_mask, const float* g_per, int B, int K, int C, int N, float weight,
                             float* per, double* total, float* g_x, float* g_latents, float* g_w, float* g_bias);

/* --------------------------------------------------------------------------
 * The latent consistency loss (EfficientZero's temporal consistency, SimSiam's
 * form, on MuZero's unrolled latents; not in main.py): the dynamics' k-th
 * latent s_k is pulled towards the representation's latent of the real board
 * at start + k, through a head of two 1x1 convs of its own, proj (C -> P) and
 * pred (P -> P).  The target side carries no gradient.
 *
 * The real boards.  mzgo_replay_window_obs_items writes, for sample (slot,
 * start, symmetry) and k = 1..unroll_steps,
 *   obs [K][B][6][N*N]   the six planes of position start + k exactly as
 *                        mzgo_replay_batch_items writes obs0 for it (the same planes
 *                        through the same sym_src permutation), STEP-major so
 *                        that [K B][6][N][N] goes to mzgo_encode as it is and
 *                        lines up with the unroll's latents 1..K
 *   window_mask [B][K]   1 where start + k <= L (row L, the final board, is
 *                        stored and counts), else 0 with all-zero planes; a
 *                        slot outside the ring gives the same
 * with mzgo_replay_ownership_items' arguments and checks: DEVICE items [B][3]
 * (nothing crosses the bus, nothing synchronises).  One launch, a workgroup per sample;
 * unroll_steps in 0..63, and 0 launches nothing (the outputs may be NULL). */
int mzgo_replay_window_obs_items(mzgo_replay* replay, const int32_t* items, int B, int unroll_steps, float* obs,
                                 float* window_mask, void* stream);

/* The representation alone: obs f32 [B][6][N][N] -> latents f32 [B][C][N][N] by
 * mzgo_unroll_forward's three representation convs, under the same parameter
 * table (any of the net's 22 tensors may be there; the representation's six
 * must be) and the same checks (C a multiple of 16, N in 2..19, emb_rows >=
 * N*N + 1).  The bits are those of the step-0 latents of mzgo_unroll_forward on
 * the same obs; no heads, no saved buffer, no gradient.  ``work``
 * (mzgo_encode_workspace bytes) holds the two intermediates.  Any B >= 1: past
 * 65535 boards the convs run in chunks inside the call.  Three launches per
 * chunk; stream-ordered; nothing allocates or synchronises. */
int mzgo_encode_workspace(int B, int C, int N, int64_t* work_bytes);
int mzgo_encode(const char* const* keys, const float* const* params, const int64_t* const* shapes, const int* ndims,
                int n_params, const float* obs, int B, int C, int N, int emb_rows, float* latents, void* work,
                int64_t work_bytes, void* stream);

/* The head and the loss on ``latents`` [K+1][B][C][N][N] (mzgo_unroll_latents'
 * layout, taken whole: step 0 takes no part), ``targets`` [K][B][C][N][N]
 * (mzgo_encode of mzgo_replay_window_obs_items' boards) and ``mask`` [B][K], with
 * proj_w [P][C], proj_b [P], pred_w [P][P], pred_b [P].  For row (k, b),
 * k = 1..K, over the D = P N N entries:
 *   u = proj(latents[k][b]),  p = pred(relu(u)),  z = proj(targets[k-1][b])
 *   cos = <p, z> / (|p| |z|)         (f64 sums; cos := 0 where |p| or |z| < 1e-8,
 *                                     and such a row's gradient is exactly 0)
 *   per[b] = weight sum_k mask[b][k-1] (1 - cos)
 * z is a constant of the backward (the stop-gradient): nothing flows to
 * ``targets`` nor, along z, to proj.  The convs are f32 fmaf chains
 * (v_mfma_f32_16x16x4_f32).  C a multiple of 16 up to 256; P one of 16, 32,
 * 48, 64; K >= 1; N in 2..19.
 * mzgo_consistency_loss writes per f32 [B] and *total (f64, the samples' sum)
 * and leaves in ``work`` what the backward reads (u, p, z and four scalars per
 * row): two launches.  mzgo_consistency_loss_backward takes the incoming g_per
 * [B] and the SAME ``work``, and writes g_latents [K+1][B][C][N][N] (step 0:
 * zeros), g_proj_w, g_proj_b, g_pred_w, g_pred_b: two launches; it reads
 * ``latents`` again and never ``targets``.  The parameter gradients' partial
 * sums are one set per chunk of rows walked in order by one workgroup, at most
 * 512 chunks and 32 MB whatever the shapes, summed over the chunks in order in
 * f64; no atomics, so repeats are bit-identical.  A row whose mask is 0 is not
 * read and contributes exact zeros.  All pointers are device pointers; nothing
 * allocates or synchronises.
 * mzgo_consistency_loss_host is both on HOST arrays with serial sums in index
 * order (csrc/mzgo_consistency.hpp's functions): no device work. */
int mzgo_consistency_loss_workspace(int B, int K, int C, int P, int N, int64_t* work_bytes);
int mzgo_consistency_loss(const float* latents, const float* targets, const float* mask, const float* proj_w,
                          const float* proj_b, const float* pred_w, const float* pred_b, int B, int K, int C, int P,
                          int N, float weight, float* per, double* total, void* work, int64_t work_bytes,
                          void* stream);
int mzgo_consistency_loss_backward(const float* latents, const float* mask, const float* g_per, const float* proj_w,
                                   const float* pred_w, int B, int K, int C, int P, int N, float weight,
                                   float* g_latents, float* g_proj_w, float* g_proj_b, float* g_pred_w,
                                   float* g_pred_b, void* work, int64_t work_bytes, void* stream);
int mzgo_consistency_loss_host(const float* latents, const float* targets, const float* mask, const float* proj_w,
                               const float* proj_b, const float* pred_w, const float* pred_b, const float* g_per,
                               int B, int K, int C, int P, int N, float weight, float* per, double* total,
                               float* g_latents, float* g_proj_w, float* g_proj_b, float* g_pred_w,
                               float* g_pred_b);

/* --------------------------------------------------------------------------
 * The trainer's optimizer tail in one call (main.py:481-484 and :379:
 * clip_grad_norm_, torch.optim.Adam.step and StepLR.step over the parameter
 * tensors, some two dozen small torch launches; this call replaces that
 * protocol for n float32 tensors of any shapes).
 *
 * An optimizer is created for n tensors of numels[i] >= 0 elements and owns,
 * on its device: a segment table (every tensor cut into chunks of
 * mzgo_optim_chunk() elements; an empty tensor has one empty chunk), one f64
 * partial per chunk, the per-tensor step counts (int64, torch's state["step"]),
 * the scheduler count, the skipped-step count and the step record.  The
 * parameters and both moments stay the caller's tensors.
 *
 * mzgo_optim_step: params / grads / exp_avg / exp_avg_sq are HOST tables of n
 * DEVICE pointers (f32, contiguous, numels[i] elements, 4-byte aligned; 16-byte
 * accesses are used per chunk where all of a chunk's pointers allow them).
 * grads[i] == NULL means tensor i has no gradient this step: it is left out of
 * the norm and stays untouched, its step count included (as torch skips a
 * parameter whose .grad is None).  The tables are read during the call and
 * travel to the kernels by value, so they may change from call to call and
 * nothing of an earlier step that is still in flight is overwritten.  Three
 * launches for n <= 96; beyond that (a) and (c) are launched once per 96
 * tensors, 2 ceil(n / 96) + 1 in all:
 *   (a) a workgroup per (tensor, chunk) sums (double)g * (double)g in a fixed
 *       order (a thread's four elements in order, then a tree over the 256
 *       threads) into its own partial; no atomics.
 *   (b) one workgroup sums the partials in index order, norm = sqrt(sum), and
 *       writes the step record {norm, coef, lr, applied} as f64[4]:
 *       applied = isfinite(norm); coef = (float)min(1, max_norm / (norm + 1e-6))
 *       (max_norm <= 0: no clipping, coef = 1); lr = lr0 * gamma **
 *       (sched_count / step_size) in f64 (integer division, integer power by
 *       squaring).  If applied, every tensor with a gradient gets step += 1 and
 *       bc1 = 1 - beta1 ** step, bc2 = 1 - beta2 ** step; else skipped += 1.
 *       sched_count += 1 on every call.
 *   (c) elementwise over the same segments, nothing when applied == 0; in f64
 *       on the f32 values, p / m / v stored rounded to f32:
 *         gc = (double)((float)g * coef)           (+ weight_decay * p, classic)
 *         m' = m + (gc - m) (1 - beta1);  v' = beta2 v + (1 - beta2) gc gc
 *         p *= 1 - lr weight_decay                 (decoupled, AdamW)
 *         p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
 *       The gradients are only READ: the clipped values are not written back,
 *       unlike clip_grad_norm_, which scales .grad in place.
 * So a non-finite gradient entry changes no parameter, moment or step count;
 * the step is refused on the device and counted.  Deterministic (the same
 * inputs give the same bits); everything is enqueued on ``stream``; no
 * allocation, no blocking copy, no synchronisation.  Calls on one optimizer
 * must be ordered (one stream, or synchronised by the caller), and the
 * optimizer's device must be current.
 *
 * mzgo_optim_record: the device address of the f64[4] record of the latest
 * step (valid until destroy; does not synchronise).
 * mzgo_optim_counts / mzgo_optim_set_counts: the step counts (HOST int64[n]),
 * the scheduler count and the skipped-step count, read or written in stream
 * order; both synchronise ``stream``.  Any out pointer of mzgo_optim_counts may
 * be NULL; mzgo_optim_set_counts takes steps_host == NULL as all zeros.
 * mzgo_optim_step_host: the host twin: the same scalar functions
 * (csrc/mzgo_optim.hpp) over HOST arrays with the same chunking and summation
 * orders, the counts passed in and out (steps int64[n], *sched, *skipped) and
 * the record written to record[4].  No device work.
 * mzgo_optim_lr: lr0 * gamma ** (sched_count / step_size), the rate the step
 * taken at that scheduler count uses.
 *
 * MZGO_EINVAL, with the reason in mzgo_last_error(), before any device work:
 *   create     n < 1; a null numels table or out; a negative numel; more than
 *              2^31 - 1 chunks in all
 *   step, step_host   a null optimizer (step) / n < 1, null numels, a negative
 *              numel, null steps, sched, skipped or record (step_host); a null
 *              params, grads, exp_avg or exp_avg_sq table; a null params[i],
 *              exp_avg[i] or exp_avg_sq[i]; a null hyper; lr0, weight_decay or
 *              gamma negative or not finite; beta1 or beta2 outside [0, 1);
 *              eps <= 0 or not finite; max_norm NaN; step_size < 1
 *   record, counts, set_counts   a null optimizer or (record) out pointer; a
 *              negative count
 *   lr         a null hyper or out; step_size < 1; sched_count < 0 */
typedef struct mzgo_optim mzgo_optim;
typedef struct mzgo_optim_hyper {
  double lr0;           /* the initial learning rate (StepLR's base) */
  double beta1, beta2;  /* Adam's betas, each in [0, 1) */
  double eps;           /* > 0 */
  double weight_decay;  /* >= 0; 0 = none */
  int decoupled;        /* weight decay: 0 = classic (Adam), 1 = decoupled (AdamW) */
  double max_norm;      /* clip_grad_norm_'s max_norm; <= 0 = no clipping */
  int64_t step_size;    /* StepLR's step_size, >= 1 */
  double gamma;         /* StepLR's gamma (1 = constant rate) */
} mzgo_optim_hyper;
int mzgo_optim_chunk(void);
int mzgo_optim_create(int n, const int64_t* numels, int device, mzgo_optim** out);
void mzgo_optim_destroy(mzgo_optim* opt);
int mzgo_optim_step(mzgo_optim* opt, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const mzgo_optim_hyper* hyper, void* stream);
int mzgo_optim_record(mzgo_optim* opt, double** dev_ptr);
int mzgo_optim_counts(mzgo_optim* opt, int64_t* steps_host, int64_t* sched, int64_t* skipped, void* stream);
int mzgo_optim_set_counts(mzgo_optim* opt, const int64_t* steps_host, int64_t sched, int64_t skipped, void* stream);
int mzgo_optim_step_host(int n, const int64_t* numels, float* const* params, const float* const* grads,
                         float* const* exp_avg, float* const* exp_avg_sq, const mzgo_optim_hyper* hyper,
                         int64_t* steps, int64_t* sched, int64_t* skipped, double* record);
int mzgo_optim_lr(const mzgo_optim_hyper* hyper, int64_t sched_count, double* lr);

#ifdef __cplusplus
}
#endif
#endif /* MZGO_H */
