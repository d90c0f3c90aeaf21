// replay_twins_check.cpp -- the replay store's two search-value host twins,
// mzgo_replay_value_targets_host and mzgo_replay_window_items_values_host, and
// the position ledger's two, mzgo_replay_sample_positions_host and
// mzgo_replay_position_priorities_host, and the game sampler's,
// mzgo_replay_sample_host
// (csrc/mzgo_replay.hip), and the item list's decode, its two row predicates and
// the plane rule the assembly kernels run (csrc/mzgo_replay.hpp: sample_window,
// window_position, window_move, observation_plane, host and device functions),
// called from a stand-alone host program so that the C
// wrappers themselves -- their vectors, the index clamp, the writes into the
// caller's buffers -- can run under AddressSanitizer and UBSan on a machine
// without a GPU.  The program links the replay unit alone: what that unit takes
// from mzgo_capi.hip is stubbed below (the twins call none of it but
// set_error), and no HIP call is made.  Every buffer has exactly the size the
// header promises, so a write or read past it is a report; results are compared
// with the rule restated here.  Exit status 0 and "ok" = clean.
//
// Build and run (host code sanitized, device code as the library's):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -x hip tools/replay_twins_check.cpp muzero-go_amd/csrc/mzgo_replay.hip -o tools/replay_twins_check
//   tools/replay_twins_check
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../include/mzgo.h"
#include "../muzero-go_amd/csrc/mzgo_replay.hpp"

// ---- mzgo_capi.hip's side of the replay unit, stubbed ----
static std::string g_err;
int mzgo::set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static void no_engine() {
  fprintf(stderr, "replay_twins_check: an engine call was reached\n");
  abort();
}
void mzgo::replay_engine_view(const mzgo_engine*, ReplayEngineView*) { no_engine(); }
bool mzgo::engine_noise_hooked(const mzgo_engine*) { no_engine(); return false; }
int mzgo::engine_play_games(mzgo_engine*, const GamesArgs&, hipStream_t) { no_engine(); return 0; }
int mzgo::engine_reanalyse_store(mzgo_engine*, const ReanalyseStoreArgs&, int, hipStream_t) { no_engine(); return 0; }
extern "C" int mzgo_reanalyse(mzgo_engine*, const int8_t*, const uint8_t*, const uint8_t*, const int32_t*, const double*,
                              int, int32_t*, double*, double*, void*) {
  no_engine();
  return 0;
}

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_err.c_str()); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// the target rule, read off mzgo.h's formula
static float restated(const std::vector<double>& r, const std::vector<double>& nu, long long i, long long n, double d) {
  const long long L = (long long)nu.size();
  double target = 0.0, factor = 1.0;
  for (long long j = i; j < i + n; ++j) {
    if (j > L) break;
    target += factor * r[j];
    factor *= d;
  }
  if (i + n <= L - 1) target += factor * nu[i + n];
  else if (i + n == L) target += factor * r[L];
  return (float)target;
}

int main() {
  srand(1);
  auto unit = [] { return rand() / (double)RAND_MAX - 0.5; };
  long targets = 0, pairs = 0;

  // ---- mzgo_replay_value_targets_host ----
  for (int L : {0, 1, 2, 7, 15, 54}) {
    std::vector<double> r(L + 1), nu(L);
    for (auto& x : r) x = rand() % 5 ? unit() : 0.0;
    for (auto& x : nu) x = rand() % 5 ? unit() : 0.0;
    for (int K : {1, 3, 10, 63})
      for (int n : {1, 3, K, K + 3, L, L + 5, INT_MAX})
        for (int start : {0, 1, L / 2, L - 1, L, L + 1, L + 70, INT_MAX - 1, INT_MAX}) {
          if (n < 1 || start < 0) continue;
          std::vector<float> out(K + 1, -7.f);              // exactly K + 1 floats
          const double d = rand() % 2 ? 0.99 : 1.0;
          CHECK(mzgo_replay_value_targets_host(r.data(), L ? nu.data() : nullptr, L, start, K, n, d, out.data()) ==
                MZGO_OK);
          for (int k = 0; k <= K; ++k) {
            const float want = restated(r, nu, (long long)start + k, n, d);
            CHECK(std::memcmp(&out[k], &want, sizeof want) == 0);
            ++targets;
          }
        }
  }
  {
    double r[2] = {1.0, 2.0}, nu[1] = {0.5};
    float out[64];
    CHECK(mzgo_replay_value_targets_host(nullptr, nu, 1, 0, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nullptr, 1, 0, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, 0, 3, 1, 0.99, nullptr) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, -1, 0, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, INT_MAX, 0, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, -1, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, INT_MIN, 3, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, 0, 0, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, 0, 64, 1, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, 0, 3, 0, 0.99, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_value_targets_host(r, nu, 1, 0, 3, INT_MIN, 0.99, out) == MZGO_EINVAL);
  }

  // ---- mzgo_replay_window_items_values_host (and, through the same builder, mzgo_replay_window_items_host) ----
  const int extremes[] = {INT_MIN, -1, 0, INT_MAX, INT_MAX - 1};
  for (int rep = 0; rep < 300; ++rep) {
    const int cap = 1 + rand() % 40, B = 1 + rand() % 300, K = 1 + rand() % 63;
    const int tds[] = {1, 2, K, K + 1, K + 2, 40, INT_MAX};
    const int td = tds[rand() % 7];
    std::vector<int32_t> length(cap), items(3 * (size_t)B);
    for (auto& x : length) x = rand() % 60;
    for (int b = 0; b < B; ++b) {
      items[3 * b] = rand() % 8 ? rand() % (cap + 2) - 1 : extremes[rand() % 5];
      items[3 * b + 1] = rand() % 8 ? rand() % 62 - 1 : extremes[rand() % 5];
      items[3 * b + 2] = rand() % 8;
    }
    for (int values = 0; values < 2; ++values) {
      // exactly the pairs the header promises: 2 B (K + 1) with value rows, B (K + 1) without
      std::vector<int32_t> out((size_t)B * (K + 1) * (values ? 2 : 1) * 2, -1);
      int32_t n = -1;
      CHECK((values ? mzgo_replay_window_items_values_host(length.data(), cap, items.data(), B, K, td, out.data(), &n)
                    : mzgo_replay_window_items_host(length.data(), cap, items.data(), B, K, out.data(), &n)) == MZGO_OK);
      // the rule restated: per sample its window and its value rows, each once; falling t, ties by batch position
      std::vector<std::pair<std::pair<int, int>, int>> want;   // ((-t, b), slot)
      for (int b = 0; b < B; ++b) {
        const long long slot = items[3 * b], start = items[3 * b + 1];
        if (slot < 0 || slot >= cap) continue;
        const long long L = length[slot];
        if (L <= 0 || start < 0 || start >= L) continue;
        std::set<long long> rows;
        for (long long t = start; t <= std::min(start + K, L - 1); ++t) rows.insert(t);
        if (values)
          for (long long t = start + td; t <= std::min(start + K + td, L - 1); ++t) rows.insert(t);
        for (long long t : rows) want.push_back({{(int)-t, b}, (int)slot});
      }
      std::sort(want.begin(), want.end());
      CHECK(n == (int32_t)want.size() && (size_t)n * 2 <= out.size());
      for (int i = 0; i < n; ++i) CHECK(out[2 * i] == want[i].second && out[2 * i + 1] == -want[i].first.first);
      pairs += n;
    }
  }
  {
    int32_t length[1] = {5}, items[3] = {0, 0, 0}, out[64], n = 0;
    CHECK(mzgo_replay_window_items_values_host(nullptr, 1, items, 1, 3, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, nullptr, 1, 3, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 3, 2, nullptr, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 3, 2, out, nullptr) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 0, items, 1, 3, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 0, 3, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 0, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 64, 2, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 3, 0, out, &n) == MZGO_EINVAL);
    CHECK(mzgo_replay_window_items_values_host(length, 1, items, 1, 3, INT_MIN, out, &n) == MZGO_EINVAL);
  }

  // ---- mzgo_replay_sample_positions_host and mzgo_replay_position_priorities_host ----
  long draws = 0, weights = 0;
  const int lens[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 130};
  for (int cap : {1, 63, 64, 65, 130, 4097})
    for (int M : {1, 64, 130, 4096}) {
      if (M == 4096 && cap > 65) continue;
      std::vector<double> w((size_t)cap * M);              // exactly [cap][M]
      std::vector<int32_t> length(cap);
      int valid = 0;
      for (int i = 0; i < cap; ++i) {
        length[i] = std::min(lens[rand() % 10] * (M == 4096 ? 31 : 1), M);
        valid += length[i] > 0;
        for (int t = 0; t < M; ++t) w[(size_t)i * M + t] = rand() % 4 ? (rand() % 1000 + 1) * 1e-3 : 0.0;
        if (length[i] > 0) w[(size_t)i * M + rand() % length[i]] = 1.0;
      }
      if (!valid) { length[0] = M; w[0] = 1.0; valid = 1; }
      for (int B : {1, valid}) {
        std::vector<int32_t> items((size_t)B * 3, -1), index(B, -1);
        std::vector<float> weight(B, -1.f);
        CHECK(mzgo_replay_sample_positions_host(w.data(), length.data(), cap, M, cap / 3, B, 5, (uint32_t)draws, 1, 0.5,
                                                items.data(), index.data(), weight.data()) == MZGO_OK);
        std::set<int> seen;
        for (int b = 0; b < B; ++b) {
          const int s = items[3 * b], t = items[3 * b + 1];
          CHECK(s >= 0 && s < cap && t >= 0 && t < length[s] && w[(size_t)s * M + t] > 0.0);
          CHECK(items[3 * b + 2] >= 0 && items[3 * b + 2] < 8 && index[b] == (s - cap / 3 + cap) % cap);
          CHECK(weight[b] > 0.f && weight[b] <= 1.f && seen.insert(s).second);
          ++draws;
        }
      }
      CHECK(mzgo_replay_sample_positions_host(w.data(), length.data(), cap, M, 0, valid + 1, 5, 0, 0, 0.0, nullptr,
                                              nullptr, nullptr) == MZGO_EINVAL);
    }
  // ---- mzgo_replay_sample_host (the same capacities; the tree is the position twin's) ----
  long game_draws = 0;
  for (int cap : {1, 63, 64, 65, 130, 4097}) {
    std::vector<double> w(cap);                            // exactly [cap]
    std::vector<int32_t> length(cap);
    int valid = 0;
    for (int i = 0; i < cap; ++i) {
      length[i] = lens[rand() % 10];
      valid += length[i] > 0;
      w[i] = (rand() % 1000 + 1) * 1e-3;
    }
    if (!valid) { length[0] = 1; valid = 1; }
    for (int B : {1, valid}) {
      std::vector<int32_t> items((size_t)B * 3, -1), index(B, -1);
      std::vector<float> weight(B, -1.f);
      CHECK(mzgo_replay_sample_host(w.data(), length.data(), cap, cap / 3, B, 5, (uint32_t)game_draws, 1, 0.5,
                                    items.data(), index.data(), weight.data()) == MZGO_OK);
      std::set<int> seen;
      for (int b = 0; b < B; ++b) {
        const int s = items[3 * b], t = items[3 * b + 1];
        CHECK(s >= 0 && s < cap && length[s] > 0 && t >= 0 && t < length[s]);
        CHECK(items[3 * b + 2] >= 0 && items[3 * b + 2] < 8 && index[b] == (s - cap / 3 + cap) % cap);
        CHECK(weight[b] > 0.f && weight[b] <= 1.f && seen.insert(s).second);
        ++game_draws;
      }
    }
    std::vector<int32_t> items((size_t)(valid + 1) * 3), index(valid + 1);
    CHECK(mzgo_replay_sample_host(w.data(), length.data(), cap, 0, valid + 1, 5, 0, 0, 0.0, items.data(), index.data(),
                                  nullptr) == MZGO_EINVAL);
    CHECK(g_err.find("exceeds") != std::string::npos);
  }
  for (int L : {0, 1, 2, 54, 4096}) {
    std::vector<double> r(L + 1), nu(L), out(L, -1.0);     // exactly L weights
    for (auto& x : r) x = unit();
    for (auto& x : nu) x = unit();
    for (int n : {1, 5, L + 3, INT_MAX})
      for (double floor : {0.0, 0.25}) {
        CHECK(mzgo_replay_position_priorities_host(r.data(), L ? nu.data() : nullptr, L, n, 0.99, 1.0, floor,
                                                   L ? out.data() : nullptr) == MZGO_OK);
        for (int t = 0; t < L; ++t) {
          const double err = std::fabs(nu[t] - (double)restated(r, nu, t, n, 0.99));
          const double fl = floor == 0.0 ? 1.17549435082228750797e-38 : floor;
          CHECK(out[t] == (err > fl ? err : fl));
          ++weights;
        }
      }
  }
  {
    double r[2] = {1.0, 2.0}, nu[1] = {0.5}, out[1];
    CHECK(mzgo_replay_position_priorities_host(nullptr, nu, 1, 1, 0.99, 1.0, 0.0, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_position_priorities_host(r, nu, 4097, 1, 0.99, 1.0, 0.0, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_position_priorities_host(r, nu, 1, 0, 0.99, 1.0, 0.0, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_position_priorities_host(r, nu, 1, 1, 0.99, 0.0, 0.0, out) == MZGO_EINVAL);
    CHECK(mzgo_replay_position_priorities_host(r, nu, 1, 1, 0.99, 1.0, -1.0, out) == MZGO_EINVAL);
  }
  // ---- sample_window, window_position, window_move, observation_plane on a store image in host memory ----
  long decoded = 0, rows_read = 0;
  {
    using namespace mzgo;
    const int N = 5, C = N * N, A = C + 1, M = 6, cap = 2;
    // exactly the ring's arrays for two slots
    std::vector<int8_t> stones((size_t)cap * (M + 1) * C);
    std::vector<uint8_t> invd((size_t)cap * (M + 1) * C), flags((size_t)cap * (M + 1));
    std::vector<int> action((size_t)cap * M), length(cap), key_gid(cap, 0);
    std::vector<double> policy((size_t)cap * M * A), reward((size_t)cap * (M + 1)), root_value((size_t)cap * M);
    for (auto& x : stones) x = (int8_t)(rand() % 3);
    for (auto& x : invd) x = (uint8_t)(rand() % 2);
    for (auto& x : flags) x = (uint8_t)(rand() % 16);
    for (auto& x : reward) x = unit();
    const Store R{N, C, A, M, cap, stones.data(), invd.data(), flags.data(), action.data(), policy.data(),
                  reward.data(), root_value.data(), length.data(), key_gid.data()};
    // two games of 4 and M moves; then lengths a store never holds, which the decode clamps to 0..M
    for (int pass = 0; pass < 2; ++pass) {
      length[0] = pass == 0 ? 4 : -2;
      length[1] = pass == 0 ? M : M + 3;
      for (int slot : {-1, 0, cap - 1, cap})
        for (int sym : {0, 7, 8, -1}) {
          // the rule restated
          const bool held = slot >= 0 && slot < cap;
          const int L = !held ? 0 : std::min(std::max(length[slot], 0), M);
          for (int start : {-1, 0, L - 1, L, L + 1}) {
            const int32_t items[6] = {77, 77, 77, slot, start, sym};     // sample b = 1
            const SampleWindow w = sample_window(R, items, 1);
            CHECK(w.slot == slot && w.start == start && w.held == held && w.L == L);
            CHECK(w.sym == (sym == 8 ? 0 : sym == -1 ? 7 : sym));
            CHECK(w.pos == (held ? (size_t)slot * (M + 1) : 0) && w.mv == (held ? (size_t)slot * M : 0));
            ++decoded;
            for (long long at = (long long)start - 2; at <= (long long)start + 66; ++at) {
              CHECK(window_position(w, at) == (held && at >= 0 && at <= L));
              CHECK(window_move(w, at) == (held && at >= 0 && at < L));
              // every row a predicate allows lies inside the image (a read past it is a report)
              if (window_position(w, at)) {
                const size_t q = w.pos + (size_t)at;
                float sum = (float)reward[q];
                for (int p = 0; p < 6; ++p)
                  for (int c = 0; c < C; ++c)
                    sum += observation_plane(R.stones + q * C, R.invd + q * C, R.flags[q], p, sym_src(N, w.sym, c));
                CHECK(sum == sum);
                ++rows_read;
              }
              if (window_move(w, at)) {
                const size_t q = w.mv + (size_t)at;
                CHECK(root_value[q] + policy[q * A + A - 1] + action[q] == 0.0);
              }
            }
          }
        }
    }
    for (long long at : {(long long)INT_MIN - 1, (long long)INT_MAX + 1, -1LL}) {
      const int32_t items[3] = {0, 0, 0};
      length[0] = M;
      const SampleWindow w = sample_window(R, items, 0);
      CHECK(!window_position(w, at) && !window_move(w, at));
    }
    // the six planes of one row under symmetry 0 (src = the cell itself), written out by hand
    const int8_t row_stones[25] = {0, 1, 2, 0, 0,  1, 1, 0, 2, 0,  0, 0, 0, 0, 2,  2, 0, 1, 0, 0,  0, 2, 2, 1, 1};
    const uint8_t row_invd[25] = {0, 1, 1, 0, 0,  1, 1, 0, 1, 1,  0, 0, 0, 0, 1,  1, 0, 1, 0, 0,  0, 1, 1, 1, 1};
    const float black[25] = {0, 1, 0, 0, 0,  1, 1, 0, 0, 0,  0, 0, 0, 0, 0,  0, 0, 1, 0, 0,  0, 0, 0, 1, 1};
    const float white[25] = {0, 0, 1, 0, 0,  0, 0, 0, 1, 0,  0, 0, 0, 0, 1,  1, 0, 0, 0, 0,  0, 1, 1, 0, 0};
    const float inval[25] = {0, 1, 1, 0, 0,  1, 1, 0, 1, 1,  0, 0, 0, 0, 1,  1, 0, 1, 0, 0,  0, 1, 1, 1, 1};
    for (int fl : {0, 1, 2, 4, 5, 8 | 2, 15}) {               // (bit 3, the fast-search bit, shows in no plane)
      const float turn = fl & 1 ? 1.f : 0.f, passed = fl & 2 ? 1.f : 0.f, done = fl & 4 ? 1.f : 0.f;
      for (int c = 0; c < 25; ++c) {
        const int src = sym_src(5, 0, c);
        CHECK(src == c);
        CHECK(observation_plane(row_stones, row_invd, fl, 0, src) == black[c]);
        CHECK(observation_plane(row_stones, row_invd, fl, 1, src) == white[c]);
        CHECK(observation_plane(row_stones, row_invd, fl, 2, src) == turn);
        CHECK(observation_plane(row_stones, row_invd, fl, 3, src) == inval[c]);
        CHECK(observation_plane(row_stones, row_invd, fl, 4, src) == passed);
        CHECK(observation_plane(row_stones, row_invd, fl, 5, src) == done);
      }
    }
  }
  printf("ok: %ld targets, %ld pairs, %ld draws, %ld game draws, %ld weights, %ld decodes, %ld rows\n", targets, pairs,
         draws, game_draws, weights, decoded, rows_read);
  return 0;
}
