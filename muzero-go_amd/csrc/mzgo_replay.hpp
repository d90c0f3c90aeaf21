// mzgo_replay.hpp -- what the device replay store (mzgo_replay.hip) shares
// with the rest of the library: the eight board symmetries as index maps
// (host and device, so that the tables a test reads are the kernel's), and the
// engine's side of the store's two engine-facing calls (mzgo_capi.hip owns
// struct mzgo_engine and the thread-local error string).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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

// mzgo_capi.hip: fill *v from an engine (no checks beyond the null pointer)
void replay_engine_view(const mzgo_engine* eng, ReplayEngineView* v);
// mzgo_capi.hip: set mzgo_last_error()'s text and return ``code``
int set_error(int code, const char* fmt, ...);

}  // namespace mzgo
