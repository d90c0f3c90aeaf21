// mzgo_capi.hip -- the C ABI of include/mzgo.h: engine lifetime, device
// memory, weight packing and dispatch to the per-(N, C) kernel tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mzgo.h"
#include "mzgo_dispatch.hpp"
#include "mzgo_replay.hpp"
#include "mzgo_tower_host.hpp"
#include "mzgo_weights.hpp"

namespace mzgo {
extern const KernelSet kernels_n5_c96, kernels_n6_c96, kernels_n9_c96, kernels_n19_c96, kernels_n6_c128,
    kernels_n6_c64;

const KernelSet* find_kernels(int N, int C) {
  static const KernelSet* all[] = {&kernels_n5_c96, &kernels_n6_c96, &kernels_n9_c96, &kernels_n19_c96,
                                   &kernels_n6_c128, &kernels_n6_c64};
  for (const KernelSet* k : all)
    if (k->N == N && k->C == C) return k;
  return nullptr;
}
}  // namespace mzgo

using namespace mzgo;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// (for the units that do not see g_err: mzgo_replay.hip)
int mzgo::set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(MZGO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

namespace {

// Reference state_dict keys (self_play.py:63-128) and their shapes.
struct Spec {
  std::string key;
  std::vector<int64_t> shape;
};

std::vector<Spec> specs(int C, int A) {
  std::vector<Spec> out;                                  // (mzgo_weights.hpp holds the keys and shapes)
  for (int k = 0; k < WK_COUNT; ++k) {
    const WeightShape sh = weight_key_shape(k, C, A);
    out.push_back(Spec{kWeightKeyNames[k], std::vector<int64_t>(sh.d, sh.d + sh.nd)});
  }
  return out;
}

}  // namespace

// CUs of the current device (one self-play workgroup fills a CU's LDS)
static int device_cus() {
  static int ncu[64];                  // per device ordinal (0: not read yet)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (ncu[dev] <= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    ncu[dev] = n;
  }
  return ncu[dev];
}

struct mzgo_engine {
  mzgo_config cfg;
  const KernelSet* ks = nullptr;
  int N = 0, C = 0, A = 0, CELLS = 0, CS = 0, G = 0, S = 0, M = 0;
  int TS = 0;                   // search-tree slots: G, or the CU count when larger (move-parallel epoch)
  std::map<std::string, std::vector<float>> sd;  // host copies of the state_dict
  std::vector<Spec> spec;
  bool dirty = true;
  bool dev_weights = false;     // d_w holds weights packed on the device (or copied): sd is empty, not missing
  WeightLayout wl;              // d_w's parts and offsets (mzgo_weights.hpp)
  float* d_w = nullptr;
  size_t d_w_bytes = 0;
  NetParams np{};
  EngineArrays E{};
  int* d_err = nullptr;
  unsigned* rq_head = nullptr;  // mzgo_reanalyse's queue head (k_reanalyse_queue)
  float* d_scr = nullptr;      // initial_inference scratch (strip boards), grown on demand
  size_t scr_floats = 0;
  std::vector<void*> allocs;
  // move-parallel launch timing (mzgo_selfplay_set_timing): per launch pair,
  // events before the boards launch, between it and k_search_queue, after it
  bool timing = false;
  std::vector<hipEvent_t> tev;
  int tn = 0;                   // launch pairs recorded since the last read
  int64_t bytes = 0;
  int epoch = 0;
  int value_cache = 0;          // the searches keep a cut batch's values (EngineArrays::cval allocated)
  int arrival_conv = 1;         // the 9x9 LDS-tree searches run a new parent's conv at its select's arrival
  const double* noise = nullptr;
  double* noise_out = nullptr;  // test hook: roots' normalised Dirichlet samples [G][M][A]
  TowerHost* tower = nullptr;   // residual-tower network (mzgo_config.tower, BASELINE config 5)

  template <class T>
  int alloc(T** p, size_t n) {
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, n * sizeof(T) + 256);
    if (e != hipSuccess) return fail(MZGO_EHIP, "hipMalloc(%zu): %s", n * sizeof(T), hipGetErrorString(e));
    allocs.push_back(v);
    bytes += (int64_t)(n * sizeof(T));
    *p = reinterpret_cast<T*>(v);
    return MZGO_OK;
  }
  ~mzgo_engine() {
    if (tower) {
      for (hipEvent_t ev : tower->evs) (void)hipEventDestroy(ev);
      tower->free_chains();
      for (void* p : {tower->d_wb, (void*)tower->d_wf, (void*)tower->ib, (void*)tower->ob, (void*)tower->s0,
                      (void*)tower->s1, (void*)tower->shp, (void*)tower->sact})
        if (p) (void)hipFree(p);
      if (tower->h_total) (void)hipHostFree(tower->h_total);
      tower->free_batch();
      delete tower;
    }
    for (hipEvent_t ev : tev) (void)hipEventDestroy(ev);
    for (void* p : allocs) (void)hipFree(p);
    if (d_w) (void)hipFree(d_w);
    if (d_scr) (void)hipFree(d_scr);
  }

  // The weight blob (reference network): allocated and zeroed at the first
  // load by either path, with NetParams pointing into it; never moved after.
  int ensure_blob() {
    if (d_w) return MZGO_OK;
    wl = weight_layout(N, C, A);
    HIPCHK(hipMalloc(&d_w, wl.total * 4));
    d_w_bytes = wl.total * 4;
    HIPCHK(hipMemset(d_w, 0, d_w_bytes));            // the parts' padding stays zero
    const float* b = d_w;
    const size_t* off = wl.off;
    np.w_conv1 = b + off[WP_CONV1_W]; np.b_conv1 = b + off[WP_CONV1_B];
    np.w_conv2 = b + off[WP_CONV2_W]; np.b_conv2 = b + off[WP_CONV2_B];
    np.w_conv3 = b + off[WP_CONV3_W]; np.b_conv3 = b + off[WP_CONV3_B];
    np.w_dyn = b + off[WP_DYN_W]; np.b_dyn = b + off[WP_DYN_B];
    np.emb = b + off[WP_EMB]; np.head_w = b + off[WP_HEAD_W]; np.etab = b + off[WP_ETAB];
    np.hs.reward_b = b + off[WP_REWARD_B]; np.hs.fc1_w = b + off[WP_FC1_W]; np.hs.fc1_b = b + off[WP_FC1_B];
    np.hs.fc2_w = b + off[WP_FC2_W]; np.hs.fc2_b = b + off[WP_FC2_B]; np.hs.value_b = b + off[WP_VALUE_B];
    np.hs.vfc_w = b + off[WP_VFC_W]; np.hs.vfc_b = b + off[WP_VFC_B]; np.hs.policy_b = b + off[WP_POLICY_B];
    np.hs.pass_logit = b + off[WP_PASS_LOGIT];
    return MZGO_OK;
  }

  // pack + upload the network if any tensor changed since the last upload
  // (nothing to do after mzgo_set_weights_device / mzgo_weights_copy until a
  // host tensor arrives; then all 22 are needed again)
  int sync_weights() {
    if (C == 0) return fail(MZGO_EINVAL, "board-only engine (latent_dim 0) has no network");
    if (!dirty) return MZGO_OK;
    for (const Spec& s : spec)
      if (!sd.count(s.key)) return fail(MZGO_ENOWEIGHTS, "missing weight '%s'", s.key.c_str());
    if (tower) {
      HIPCHK(tower->upload(sd));
      dirty = false;
      return MZGO_OK;
    }
    if (int rc = ensure_blob()) return rc;
    const float* src[WK_COUNT];
    for (int k = 0; k < WK_COUNT; ++k) src[k] = sd[spec[k].key].data();
    std::vector<float> blob(wl.total, 0.f);
    pack_weights_host(wl, src, blob.data());
    HIPCHK(hipMemcpy(d_w, blob.data(), wl.total * 4, hipMemcpyHostToDevice));
    dev_weights = false;
    dirty = false;
    return MZGO_OK;
  }

  // drop-in inference scratch of the tower engine for B boards (zero borders)
  int tower_scratch(int B) {
    TowerHost& t = *tower;
    if (B <= t.scap) return MZGO_OK;
    for (void* p : {(void*)t.ib, (void*)t.ob, (void*)t.s0, (void*)t.s1, (void*)t.shp, (void*)t.sact})
      if (p) HIPCHK(hipFree(p));
    t.ib = t.ob = t.s0 = t.s1 = nullptr; t.shp = nullptr; t.sact = nullptr; t.scap = 0;
    const size_t n = (size_t)B * t.slot();
    for (bf16** q : {&t.ib, &t.ob, &t.s0, &t.s1}) {
      HIPCHK(hipMalloc((void**)q, n * sizeof(bf16)));
      HIPCHK(hipMemset(*q, 0, n * sizeof(bf16)));
    }
    HIPCHK(hipMalloc((void**)&t.shp, (size_t)B * t.CC * 3 * t.CS * sizeof(float)));
    HIPCHK(hipMalloc((void**)&t.sact, (size_t)B * sizeof(int)));
    t.scap = B;
    return MZGO_OK;
  }

  SearchParams search_params() const {
    SearchParams sp;
    sp.c_puct = cfg.c_puct; sp.discount = cfg.discount;
    sp.dirichlet_alpha = cfg.dirichlet_alpha; sp.dirichlet_epsilon = cfg.dirichlet_epsilon;
    sp.pass_epsilon = cfg.pass_epsilon; sp.num_simulations = S; sp.compat = cfg.compat;
    sp.variant = cfg.search_variant;
    sp.factored = cfg.direct_dynamics ? 0 : 1;
    sp.seed = cfg.seed;
    sp.helpers = 0;
    sp.net = 0;
    sp.tail = 0;
    const char* lz = getenv("MZGO_LAZY_ROWS");        // (=0: eager rows in self-play too, an A/B switch)
    sp.lazy_rows = lz && atoi(lz) == 0 ? 0 : 1;
    sp.value_cache = value_cache;
    sp.arrival_conv = arrival_conv;
    sp.fast_simulations = 0;                          // searches, reanalysis, the arena: always S
    sp.full_search_prob = 1.0;
    return sp;
  }
  // ... of a self-play launch: the playout caps of the configuration (move_budget, mzgo_move.hpp)
  SearchParams selfplay_params() const {
    SearchParams sp = search_params();
    if (!tower && cfg.full_search_prob < 1.0) {       // (p = 1: every move is full, the caps are off)
      sp.fast_simulations = cfg.fast_simulations;
      sp.full_search_prob = cfg.full_search_prob;
    }
    return sp;
  }
};

// the device replay store's view of an engine's finished games (mzgo_replay.hip)
void mzgo::replay_engine_view(const mzgo_engine* e, ReplayEngineView* v) {
  const EngineArrays& E = e->E;
  *v = ReplayEngineView{e->N, e->G, e->M, e->C, e->tower ? 1 : 0, e->cfg.game_base, e->epoch,
                        E.stones, E.invd, E.meta, E.rec_stones, E.rec_invd, E.rec_flags, E.rec_action,
                        E.rec_value, E.rec_policy, E.rec_reward, E.final_reward};
}

extern "C" {

const char* mzgo_last_error(void) { return g_err.c_str(); }

void mzgo_default_config(mzgo_config* c, int N) {
  std::memset(c, 0, sizeof *c);
  c->board_size = N;
  c->latent_dim = 96;
  c->num_games = 1;
  c->num_simulations = 128;
  c->max_moves = N * N;
  c->compat = 0;
  c->temperature_moves = 15;
  c->c_puct = 2.5;
  c->discount = 0.99;
  c->dirichlet_alpha = 0.15;
  c->dirichlet_epsilon = 0.02;
  c->pass_epsilon = 0.01;
  c->temperature = 1.0;
  c->komi = 0.0;
  c->seed = 1234;
  c->fast_simulations = 0;
  c->full_search_prob = 1.0;
}

int mzgo_playout_budget_host(uint64_t seed, uint32_t key_gid, int move, int num_simulations, int fast_simulations,
                             double full_search_prob, int* budget) {
  if (!budget) return fail(MZGO_EINVAL, "mzgo_playout_budget_host: null budget");
  if (num_simulations < 1 || move < 0)
    return fail(MZGO_EINVAL, "mzgo_playout_budget_host: num_simulations %d must be >= 1 and move %d >= 0",
                num_simulations, move);
  if (fast_simulations < 0 || fast_simulations > num_simulations)
    return fail(MZGO_EINVAL, "fast_simulations must be in 0..num_simulations (%d), got %d", num_simulations,
                fast_simulations);
  if (!(full_search_prob >= 0.0 && full_search_prob <= 1.0))
    return fail(MZGO_EINVAL, "full_search_prob must be in [0, 1], got %g", full_search_prob);
  SearchParams sp{};
  sp.seed = seed;
  sp.num_simulations = num_simulations;
  sp.fast_simulations = fast_simulations;
  sp.full_search_prob = full_search_prob;
  *budget = playout_budget(sp, key_gid, move);
  return MZGO_OK;
}

int mzgo_engine_create(const mzgo_config* cfg, mzgo_engine** out) {
  if (!cfg || !out) return fail(MZGO_EINVAL, "null argument");
  *out = nullptr;
  const int N = cfg->board_size, C = cfg->latent_dim;
  const int TW = cfg->tower, RB = cfg->res_blocks;
  if (TW != 0 && TW != 1) return fail(MZGO_EINVAL, "tower must be 0 (reference network) or 1 (residual tower)");
  if (TW && RB < 0) return fail(MZGO_EINVAL, "res_blocks must be >= 0");
  const TowerSet* tset = nullptr;
  if (TW) {
    // the residual-tower network (BASELINE config 5): board kernels of the
    // N x N build, the tower's own conv / tree kernels
    tset = find_tower(N);
    if (!tset) return fail(MZGO_EINVAL, "unsupported board_size %d for the tower network (built: 5, 9, 19)", N);
    if (C < 64 || C % 64 != 0 || C > 1024)
      return fail(MZGO_EINVAL, "the tower network needs latent_dim a multiple of 64 in [64, 1024], got %d", C);
  }
  const KernelSet* ks = find_kernels(N, (C == 0 || TW) ? 96 : C);
  if (!ks) return fail(MZGO_EINVAL, "unsupported board_size %d / latent_dim %d (built: N in {5,6,9,19} with C=96; N=6 with C=128 or 64)", N, C);
  if (cfg->num_games < 1) return fail(MZGO_EINVAL, "num_games must be >= 1");
  if (C != 0 && cfg->num_simulations < 1) return fail(MZGO_EINVAL, "num_simulations must be >= 1");
  if (cfg->compat != 0 && cfg->compat != 1) return fail(MZGO_EINVAL, "compat must be 0 or 1");
  if (C != 0) {                                       // (board-only engines search nothing: both fields ignored)
    if (cfg->fast_simulations < 0 || cfg->fast_simulations > cfg->num_simulations)
      return fail(MZGO_EINVAL, "fast_simulations must be in 0..num_simulations (%d), got %d", cfg->num_simulations,
                  cfg->fast_simulations);
    if (!(cfg->full_search_prob >= 0.0 && cfg->full_search_prob <= 1.0))
      return fail(MZGO_EINVAL, "full_search_prob must be in [0, 1], got %g", cfg->full_search_prob);
    if (TW && cfg->fast_simulations > 0)
      return fail(MZGO_EINVAL, "fast_simulations > 0 (playout cap randomization) is not supported on tower engines");
  }
  if (cfg->direct_dynamics != 0 && cfg->direct_dynamics != 1)
    return fail(MZGO_EINVAL, "direct_dynamics must be 0 (factored expansion) or 1 (a conv per simulation)");
  if (cfg->search_variant != 0 && cfg->search_variant != 1)
    return fail(MZGO_EINVAL, "search_variant must be 0 (self_play.py) or 1 (main.py)");
  HIPCHK(hipSetDevice(cfg->device));
  auto* e = new mzgo_engine();
  e->cfg = *cfg;
  e->ks = ks;
  e->N = N; e->C = C; e->A = N * N + 1; e->CELLS = N * N; e->CS = (N * N + 15) / 16 * 16;
  e->G = cfg->num_games;
  e->S = C == 0 ? 0 : cfg->num_simulations;
  e->M = cfg->max_moves > 0 ? cfg->max_moves : N * N;
  e->cfg.max_moves = e->M;
  if (TW) {
    e->spec.clear();
    for (auto& kv : TowerHost::specs(C, e->A, RB)) e->spec.push_back(Spec{kv.first, kv.second});
  } else {
    e->spec = specs(C, e->A);
  }
  EngineArrays& E = e->E;
  E.S = e->S;
  E.max_moves = e->M;
  // Search-tree slots.  Boards whose game-per-workgroup launch takes helper
  // workgroups (19x19: fewer games than CUs, 3 helpers each) get a tree per
  // CU when the move-parallel epoch can run (compat "reference", self_play.py
  // search): its queue runs one search per CU (k_search_queue).
  // MZGO_MOVE_PARALLEL=0 at creation keeps G.
  e->TS = e->G;
  if (C != 0 && !TW && ks->shared_batches && cfg->compat == 0 && cfg->search_variant == 0) {
    const char* v = getenv("MZGO_MOVE_PARALLEL");
    if (!(v && atoi(v) == 0)) e->TS = std::max(e->G, device_cus());
  }
  const size_t G = e->G, TSL = e->TS, n1 = (size_t)e->S + 1, A = e->A, CELLS = e->CELLS, M = e->M;
  int rc = MZGO_OK;
  auto chk = [&](int r) { if (r != MZGO_OK && rc == MZGO_OK) rc = r; };
  if (C != 0 && !TW) {
    // S+1 node slots + one scratch latent per game
    chk(e->alloc(&E.pool, TSL * (n1 + 1) * (size_t)C * e->CS));
    // pad cells (>= N*N) of pooled latents are read as zeros and never written
    if (rc == MZGO_OK && hipMemset(E.pool, 0, TSL * (n1 + 1) * (size_t)C * e->CS * sizeof(float)) != hipSuccess)
      chk(fail(MZGO_EHIP, "hipMemset(pool) failed"));
  }
  if (TW) {
    TowerHost* t = e->tower = new TowerHost();
    t->ts = tset;
    t->N = N; t->C = C; t->CC = C / 64; t->blocks = RB; t->G = e->G; t->S = e->S; t->A = e->A;
    t->P = (N + 2) * (N + 2); t->CS = e->CS;
    TowerArrays& T = t->TA;
    T.C = C; T.co_chunks = C / 64;
    const size_t slot = (size_t)t->slot();
    // batched simulation steps (MZGO_TOWER_BATCH=1): up to min(A, S) pending
    // entries per game (the root's children), so up to G x that many boards
    // per step; their buffers are allocated on first use (ensure_batch)
    t->bq_cap = (int)std::min<size_t>(A, n1 - 1);
    t->maxb = (int)(G * (size_t)t->bq_cap);
    T.bq_cap = t->bq_cap;
    // node latents (bf16, zero borders: the conv's padding is never written);
    // the tower's two scratch activations per board of a one-leaf step
    chk(e->alloc(&T.pool, G * n1 * slot));
    chk(e->alloc(&t->t0, G * slot));
    chk(e->alloc(&t->t1, G * slot));
    chk(e->alloc(&T.rep_in, G * (size_t)t->P * 64));
    if (rc == MZGO_OK) {
      for (auto pr : {std::make_pair((void*)T.pool, G * n1 * slot), std::make_pair((void*)t->t0, G * slot),
                      std::make_pair((void*)t->t1, G * slot), std::make_pair((void*)T.rep_in, G * (size_t)t->P * 64)})
        if (hipMemset(pr.first, 0, pr.second * sizeof(bf16)) != hipSuccess) chk(fail(MZGO_EHIP, "hipMemset(tower) failed"));
    }
    T.slot = (long long)slot;
    chk(e->alloc(&T.hpart, G * (size_t)t->CC * 3 * e->CS));
    chk(e->alloc(&T.bq_n, G));
    chk(e->alloc(&T.bq_nid0, G));
    chk(e->alloc(&T.nbg, G));
    chk(e->alloc(&T.b_total, 1));
    if (rc == MZGO_OK && (hipMemset(T.bq_n, 0, G * sizeof(int)) != hipSuccess ||
                          hipHostMalloc(&t->h_total, sizeof(int), hipHostMallocDefault) != hipSuccess))
      chk(fail(MZGO_EHIP, "tower batch setup failed"));
    chk(e->alloc(&T.rootmask, G * A));
    chk(e->alloc(&T.passp, G));
    chk(e->alloc(&T.key, G));
    chk(e->alloc(&T.playing, G));
    chk(e->alloc(&T.evalact, G));
    chk(e->alloc(&T.in_idx, G));
    chk(e->alloc(&T.out_idx, G));
    chk(e->alloc(&T.root_idx, G));
    chk(e->alloc(&T.act, G));
    chk(e->alloc(&T.job, G * 3));
    chk(e->alloc(&T.simc, G));
    if (rc == MZGO_OK) {
      std::vector<int> ri(G);
      for (size_t g = 0; g < G; ++g) ri[g] = (int)(g * n1);
      if (hipMemcpy(T.root_idx, ri.data(), G * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemset(T.playing, 0, G * sizeof(int)) != hipSuccess || hipMemset(T.evalact, 0, G * sizeof(int)) != hipSuccess)
        chk(fail(MZGO_EHIP, "tower index setup failed"));
    }
  }
  if (C != 0) {
    chk(e->alloc(&E.prior, TSL * n1 * A));
    chk(e->alloc(&E.child, TSL * n1 * A));
    chk(e->alloc(&E.visits, TSL * n1));
    chk(e->alloc(&E.wsum, TSL * n1));
    chk(e->alloc(&E.root_prior, TSL * A));
    chk(e->alloc(&E.path, TSL * (n1 + 1)));
    chk(e->alloc(&E.nodes, TSL));
    chk(e->alloc(&E.nact, TSL * n1));
    // the value cache of the LDS trees' speculative batches (sim_loop): only
    // engines whose searches take that path (MZGO_VALUE_CACHE=0: off, an A/B switch)
    const char* vc = getenv("MZGO_VALUE_CACHE");
    e->value_cache = !TW && !cfg->direct_dynamics && ks->value_cache_cap > 0 && e->S + 2 <= ks->value_cache_cap &&
                     !(vc && atoi(vc) == 0);
    if (e->value_cache) chk(e->alloc(&E.cval, TSL * n1 * A));
    // the arrival conv of the 9x9 LDS-tree searches (sim_loop; MZGO_ARRIVAL_CONV=0: today's
    // order of select and conv, an A/B switch; 1, the default, or more: the conv first.  The
    // value 2 was the batch's picks under the conv as well, measured slower and taken out
    // again, DESIGN §7: it means 1)
    const char* ac = getenv("MZGO_ARRIVAL_CONV");
    e->arrival_conv = !(ac && atoi(ac) <= 0);
    chk(e->alloc(&E.jobs, TSL * job_bytes(A)));
    chk(e->alloc(&E.mpq, 2 * (size_t)G + 1));
    chk(e->alloc(&E.rec_stones, G * M * CELLS));
    chk(e->alloc(&E.rec_invd, G * M * CELLS));
    chk(e->alloc(&E.rec_flags, G * M));
    chk(e->alloc(&E.rec_action, G * M));
    chk(e->alloc(&E.rec_value, G * M));
    chk(e->alloc(&E.rec_policy, G * M * A));
    chk(e->alloc(&E.rec_reward, G * M));
  }
  chk(e->alloc(&E.stones, G * CELLS));
  chk(e->alloc(&E.invd, G * CELLS));
  chk(e->alloc(&E.meta, G * 4));
  chk(e->alloc(&E.game_len, G));
  chk(e->alloc(&E.final_reward, G));
  chk(e->alloc(&E.status, G));
  chk(e->alloc(&E.counters, kCounters));
  chk(e->alloc(&e->d_err, 1));
  chk(e->alloc(&e->rq_head, 1));
#ifdef MZGO_STAMPS
  chk(e->alloc(&E.stamps, TSL * kStampPhases));
  if (E.stamps) (void)hipMemset(E.stamps, 0, TSL * kStampPhases * 8);
#endif
  if (rc != MZGO_OK) { delete e; return rc; }
  if (hipMemset(E.counters, 0, kCounters * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(e->d_err, 0, sizeof(int)) != hipSuccess) {
    delete e;
    return fail(MZGO_EHIP, "hipMemset failed");
  }
  hipError_t he = ks->board_reset(E, e->G, nullptr);
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) { delete e; return fail(MZGO_EHIP, "board reset: %s", hipGetErrorString(he)); }
  *out = e;
  return MZGO_OK;
}

void mzgo_engine_destroy(mzgo_engine* e) { delete e; }

int64_t mzgo_engine_device_bytes(const mzgo_engine* e) { return e ? e->bytes + (int64_t)e->d_w_bytes : 0; }

int mzgo_set_weights(mzgo_engine* e, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!e || !key || !data || (!shape && ndim > 0)) return fail(MZGO_EINVAL, "null argument");
  for (const Spec& s : e->spec) {
    if (s.key != key) continue;
    if ((int)s.shape.size() != ndim) return fail(MZGO_EINVAL, "'%s': expected %zu dims, got %d", key, s.shape.size(), ndim);
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] != s.shape[i])
        return fail(MZGO_EINVAL, "'%s': dim %d is %lld, expected %lld", key, i, (long long)shape[i], (long long)s.shape[i]);
      n *= (size_t)shape[i];
    }
    e->sd[key].assign(data, data + n);
    e->dirty = true;
    return MZGO_OK;
  }
  return fail(MZGO_EINVAL, "unexpected key '%s' in state_dict", key);
}

int mzgo_weights_ready(const mzgo_engine* e) {
  if (!e || e->C == 0) return 0;
  if (e->dev_weights && !e->dirty) return 1;
  for (const Spec& s : e->spec)
    if (!e->sd.count(s.key)) return 0;
  return 1;
}

int mzgo_set_weights_device(mzgo_engine* e, const char* const* keys, const float* const* data_dev,
                            const int64_t* const* shapes, const int* ndims, int n, void* stream) {
  if (!e) return fail(MZGO_EINVAL, "mzgo_set_weights_device: null argument");
  if (e->C == 0) return fail(MZGO_EINVAL, "mzgo_set_weights_device: board-only engine (latent_dim 0) has no network");
  if (e->tower) return fail(MZGO_EINVAL, "mzgo_set_weights_device: tower engines (tower = 1) are not supported");
  const float* src[WK_COUNT];
  if (int rc = weight_table("mzgo_set_weights_device", keys, data_dev, shapes, ndims, n, e->C, e->A, src)) return rc;
  if (int rc = e->ensure_blob()) return rc;
  HIPCHK(pack_weights_device(e->wl, src, e->d_w, (hipStream_t)stream));
  e->sd.clear();                                      // the host copies are stale
  e->dirty = false;
  e->dev_weights = true;
  return MZGO_OK;
}

int mzgo_weights_copy(mzgo_engine* dst, const mzgo_engine* src_c, void* stream) {
  mzgo_engine* src = const_cast<mzgo_engine*>(src_c);   // (its pending host tensors are packed first)
  if (!dst || !src) return fail(MZGO_EINVAL, "mzgo_weights_copy: null engine");
  if (dst->C == 0 || src->C == 0)
    return fail(MZGO_EINVAL, "mzgo_weights_copy: board-only engine (latent_dim 0) has no network");
  if (dst->tower || src->tower) return fail(MZGO_EINVAL, "mzgo_weights_copy: tower engines (tower = 1) are not supported");
  if (dst->N != src->N || dst->C != src->C)
    return fail(MZGO_EINVAL, "mzgo_weights_copy: engines differ (board_size %d / latent_dim %d from %d / %d)", dst->N,
                dst->C, src->N, src->C);
  if (int rc = src->sync_weights()) return rc;          // MZGO_ENOWEIGHTS when src was never loaded
  if (dst == src) return MZGO_OK;
  if (int rc = dst->ensure_blob()) return rc;
  HIPCHK(hipMemcpyAsync(dst->d_w, src->d_w, src->wl.total * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  dst->sd.clear();
  dst->dirty = false;
  dst->dev_weights = true;
  return MZGO_OK;
}

int mzgo_weights_export(mzgo_engine* e, float* data_host, int64_t cap, int64_t* n_floats, void* stream) {
  if (!e || !n_floats) return fail(MZGO_EINVAL, "mzgo_weights_export: null argument");
  if (e->C == 0) return fail(MZGO_EINVAL, "mzgo_weights_export: board-only engine (latent_dim 0) has no network");
  if (e->tower) return fail(MZGO_EINVAL, "mzgo_weights_export: tower engines (tower = 1) are not supported");
  if (int rc = e->sync_weights()) return rc;
  *n_floats = (int64_t)e->wl.total;
  if (!data_host) return MZGO_OK;
  if (cap < *n_floats)
    return fail(MZGO_EINVAL, "mzgo_weights_export: cap %lld < %lld floats", (long long)cap, (long long)*n_floats);
  HIPCHK(hipMemcpyAsync(data_host, e->d_w, e->wl.total * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_initial_inference(mzgo_engine* e, const float* obs, int B, float* latent, float* value,
                           float* logits, void* stream) {
  if (!e || !obs || !latent || !value || !logits || B < 1) return fail(MZGO_EINVAL, "bad argument");
  int rc = e->sync_weights();
  if (rc) return rc;
  if (e->tower) {
    if ((rc = e->tower_scratch(B))) return rc;
    TowerHost& t = *e->tower;
    hipStream_t s = (hipStream_t)stream;
    TowerArrays Tb = t.TA;
    Tb.hpart = t.shp;
    HIPCHK(t.ts->tin(obs, t.ib, B, t.C, 1, t.slot(), s));
    HIPCHK(t.tower(t.rep, t.ib, nullptr, t.slot(), t.ob, nullptr, t.slot(), nullptr, nullptr, B, t.s0, t.s1, t.shp, s));
    HIPCHK(t.ts->tout(t.ob, latent, B, t.C, s));
    HIPCHK(t.ts->theads(Tb, B, 0, nullptr, value, logits, s));
    return MZGO_OK;
  }
  float* scr = nullptr;
  if (e->ks->rep_scratch) {
    const size_t need = (size_t)B * e->ks->rep_scratch;
    if (need > e->scr_floats) {
      if (e->d_scr) HIPCHK(hipFree(e->d_scr));   // synchronising: no launch still reads it
      e->d_scr = nullptr;
      e->scr_floats = 0;
      HIPCHK(hipMalloc(&e->d_scr, need * sizeof(float)));
      e->scr_floats = need;
    }
    scr = e->d_scr;
  }
  HIPCHK(e->ks->initial_inference(e->np, obs, B, latent, value, logits, scr, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_recurrent_inference(mzgo_engine* e, const float* latent, const int64_t* action, int B,
                             float* next_latent, float* reward, float* value, float* logits, void* stream) {
  if (!e || !latent || !action || !next_latent || !reward || !value || !logits || B < 1)
    return fail(MZGO_EINVAL, "bad argument");
  int rc = e->sync_weights();
  if (rc) return rc;
  if (e->tower) {
    if ((rc = e->tower_scratch(B))) return rc;
    TowerHost& t = *e->tower;
    hipStream_t s = (hipStream_t)stream;
    TowerArrays Tb = t.TA;
    Tb.hpart = t.shp;
    HIPCHK(launch_tact(action, t.sact, B, e->A, e->d_err, s));
    HIPCHK(t.ts->tin(latent, t.ib, B, t.C, 0, t.slot(), s));
    HIPCHK(t.tower(t.dyn, t.ib, nullptr, t.slot(), t.ob, nullptr, t.slot(), t.sact, nullptr, B, t.s0, t.s1, t.shp, s));
    HIPCHK(t.ts->tout(t.ob, next_latent, B, t.C, s));
    HIPCHK(t.ts->theads(Tb, B, 1, reward, value, logits, s));
    return MZGO_OK;
  }
  HIPCHK(e->ks->recurrent_inference(e->np, latent, action, B, next_latent, reward, value, logits,
                                    e->d_err, (hipStream_t)stream));
  return MZGO_OK;
}

// Tower engines: a k_tconv_chain wait that expired makes that launch's
// results wrong; it is reported (MZGO_EHIP) and cleared by the first API
// call that synchronises afterwards -- every call of the tower path does
// (self-play moves, search, inference checks, tree / record / counter reads).
static int check_chain(mzgo_engine* e, hipStream_t s) {
  if (!e->tower) return MZGO_OK;
  bool bad = false;
  HIPCHK(e->tower->chain_error(s, bad));
  if (bad) return fail(MZGO_EHIP, "k_tconv_chain: a workgroup's wait for its board expired (results of the call are wrong)");
  return MZGO_OK;
}

int mzgo_check_inference_errors(mzgo_engine* e, void* stream) {
  if (!e) return fail(MZGO_EINVAL, "null engine");
  if (int rc = check_chain(e, (hipStream_t)stream)) return rc;
  int h = 0;
  HIPCHK(hipMemcpyAsync(&h, e->d_err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (h) {
    HIPCHK(hipMemsetAsync(e->d_err, 0, sizeof(int), (hipStream_t)stream));
    return fail(MZGO_EINVAL, "index out of range in self (action outside [0, %d))", e->A);
  }
  return MZGO_OK;
}

int mzgo_search(mzgo_engine* e, const float* root_obs, const double* noise, int G, int move_index,
                int32_t* visits, double* value, void* stream) {
  if (!e || !root_obs || G < 1 || G > e->G) return fail(MZGO_EINVAL, "bad argument (G=%d, engine has %d slots)", G, e ? e->G : 0);
  int rc = e->sync_weights();
  if (rc) return rc;
  if (e->tower) {
    TowerHost& t = *e->tower;
    hipStream_t s = (hipStream_t)stream;
    const SearchParams sp = e->search_params();
    HIPCHK(hipMemsetAsync(t.TA.playing, 0, e->G * sizeof(int), s));
    HIPCHK(t.ts->obs_search(t.TA, sp, root_obs, e->cfg.game_base, move_index, G, s));
    HIPCHK(t.root_phase(sp, e->E, noise, e->A, 0, s));
    HIPCHK(t.simulations(sp, e->E, s));
    HIPCHK(t.ts->search_out(t.TA, sp, e->E, G, visits, value, s));
    return check_chain(e, s);
  }
  SearchParams sp = e->search_params();
  sp.lazy_rows = 0;                                   // every row of an exported tree formed
  HIPCHK(e->ks->search(e->np, sp, e->E, root_obs, noise, G, e->cfg.game_base, move_index, visits, value,
                       (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_reanalyse(mzgo_engine* e, const int8_t* stones, const uint8_t* invd, const uint8_t* flags,
                   const int32_t* ids, const double* noise, int n, int32_t* visits, double* value, double* policy,
                   void* stream) {
  if (!e) return fail(MZGO_EINVAL, "mzgo_reanalyse: null engine");
  if (n < 1) return fail(MZGO_EINVAL, "mzgo_reanalyse: n must be >= 1, got %d", n);
  if (!stones || !invd || !flags || !ids || !visits || !value)
    return fail(MZGO_EINVAL, "mzgo_reanalyse: null %s",
                !stones ? "stones" : !invd ? "invd" : !flags ? "flags" : !ids ? "ids" : !visits ? "visits" : "value");
  if (e->C == 0) return fail(MZGO_EINVAL, "mzgo_reanalyse: board-only engine (latent_dim 0) has no network");
  if (e->tower) return fail(MZGO_EINVAL, "mzgo_reanalyse: tower engines (tower = 1) are not supported");
  int rc = e->sync_weights();
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const SearchParams sp = e->search_params();          // (self-play's row laziness; no helpers, network 0)
  const int ncu = device_cus();
  int wg = ncu > 0 && ncu < e->TS ? ncu : e->TS;       // one tree slot per workgroup
  if (n < wg) wg = n;
  const ReanalyseArgs ra{stones, invd, flags, ids, noise, n, e->rq_head, visits, value, policy};
  HIPCHK(hipMemsetAsync(e->rq_head, 0, sizeof(unsigned), s));
  HIPCHK(e->ks->reanalyse(e->np, sp, e->E, ra, wg, s));
  return MZGO_OK;
}

int mzgo_tree_export(mzgo_engine* e, int g, int32_t* n_nodes, int32_t* child, int32_t* visits,
                     double* value_sum, float* prior, double* root_prior, void* stream) {
  if (!e || e->C == 0 || g < 0 || g >= e->G) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t n1 = (size_t)e->S + 1, A = e->A;
  if (e->tower) {
    // rows a select never reached still hold logits + the kRawRow sentinel
    // after a self-play move (lazy child priors): settle them as the search
    // API does (k_tsearch_out; idempotent, the values a later select would form)
    TowerHost& t = *e->tower;
    HIPCHK(t.ts->search_out(t.TA, e->search_params(), e->E, e->G, nullptr, nullptr, s));
    if (int rc = check_chain(e, s)) return rc;
  }
  int nn = 0;
  HIPCHK(hipMemcpyAsync(&nn, e->E.nodes + g, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (n_nodes) *n_nodes = nn;
  if (child) HIPCHK(hipMemcpyAsync(child, e->E.child + g * n1 * A, nn * A * 4, hipMemcpyDeviceToHost, s));
  if (visits) HIPCHK(hipMemcpyAsync(visits, e->E.visits + g * n1, nn * 4, hipMemcpyDeviceToHost, s));
  if (value_sum) HIPCHK(hipMemcpyAsync(value_sum, e->E.wsum + g * n1, nn * 8, hipMemcpyDeviceToHost, s));
  if (prior) HIPCHK(hipMemcpyAsync(prior, e->E.prior + g * n1 * A, nn * A * 4, hipMemcpyDeviceToHost, s));
  if (root_prior) HIPCHK(hipMemcpyAsync(root_prior, e->E.root_prior + g * A, A * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return MZGO_OK;
}

int mzgo_board_reset(mzgo_engine* e, void* stream) {
  if (!e) return fail(MZGO_EINVAL, "null engine");
  HIPCHK(e->ks->board_reset(e->E, e->G, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_board_step(mzgo_engine* e, const int32_t* actions, int32_t* status, double* winner, void* stream) {
  if (!e || !actions) return fail(MZGO_EINVAL, "bad argument");
  HIPCHK(e->ks->board_step(e->E, e->G, actions, status, winner, e->cfg.komi, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_board_planes(mzgo_engine* e, double* planes, void* stream) {
  if (!e || !planes) return fail(MZGO_EINVAL, "bad argument");
  HIPCHK(e->ks->board_planes(e->E, e->G, planes, (hipStream_t)stream));
  return MZGO_OK;
}

int mzgo_board_set(mzgo_engine* e, int g, const int8_t* stones, const uint8_t* invd, const int32_t* meta,
                   void* stream) {
  if (!e || g < 0 || g >= e->G || !stones || !invd || !meta) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(e->E.stones + (size_t)g * e->CELLS, stones, e->CELLS, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(e->E.invd + (size_t)g * e->CELLS, invd, e->CELLS, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(e->E.meta + (size_t)g * 4, meta, 16, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return MZGO_OK;
}

int mzgo_selfplay_reset(mzgo_engine* e, int epoch, void* stream) {
  if (!e || e->C == 0) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  e->epoch = epoch;
  HIPCHK(e->ks->board_reset(e->E, e->G, s));
  return MZGO_OK;
}

// k_selfplay_move; boards whose batch expansions stream Y from L2 (19x19) get
// helper workgroups, 3 per game by default (MZGO_HELPERS_PER_GAME), with the
// job slots zeroed before the launch (batch_expand_shared)

// The epoch tail (whole-game launches): a workgroup whose game has ended
// stays resident and serves running games.  Only when every workgroup of the
// launch is resident at once (one per CU): otherwise ended workgroups would
// hold CUs that games not yet dispatched are waiting for.  MZGO_TAIL_HELPERS=0
// turns it off, =2 forces it on past that bound (a test of the kernel's own
// guards: helpers never join a game whose workgroup has not started).  The
// bound is per launch: engines launched concurrently on several streams (bench.py
// --refill) share the CUs, so their launches are not all resident even when
// each fits -- the started guard keeps that correct, but ended workgroups then
// hold CUs the other engines' games need, and --refill sets MZGO_TAIL_HELPERS=0.
static bool tail_enabled(int workgroups) {
  const char* v = getenv("MZGO_TAIL_HELPERS");
  const int mode = v ? atoi(v) : 1;
  if (mode == 0) return false;
  return mode == 2 || workgroups <= device_cus();
}

// The move-parallel epoch (k_search_queue): multi-move launches under compat
// "reference" play the boards first and then run every recorded move's search
// from one queue, one workgroup per CU (no helper workgroups: at 19x19 every
// CU runs its own search instead of a game's 4 workgroups sharing one); the
// records are the same as the game-per-workgroup launch's.
// MZGO_MOVE_PARALLEL=0 keeps the game-per-workgroup launch (its epoch tail:
// tail_help / join_running_game).
static bool move_parallel(const mzgo_engine* e, const SearchParams& sp, const PlayParams& pp) {
  const char* v = getenv("MZGO_MOVE_PARALLEL");
  if (v && atoi(v) == 0) return false;
  return pp.moves > 1 && !pp.arena && sp.compat == 0 && sp.variant == 0;
}

static int launch_selfplay(mzgo_engine* e, const NetParams& np_b, const PlayParams& pp, hipStream_t s) {
  SearchParams sp = pp.arena ? e->search_params() : e->selfplay_params();   // (the arena: no playout caps)
  if (move_parallel(e, sp, pp)) {
    hipEvent_t* ev = nullptr;
    if (e->timing) {
      while ((int)e->tev.size() < 3 * (e->tn + 1)) {
        hipEvent_t x;
        HIPCHK(hipEventCreate(&x));
        e->tev.push_back(x);
      }
      ev = &e->tev[3 * e->tn++];
    }
    HIPCHK(hipMemsetAsync(e->E.mpq + 2 * e->G, 0, sizeof(int), s));
    if (ev) HIPCHK(hipEventRecord(ev[0], s));
    HIPCHK(e->ks->selfplay_boards(sp, pp, e->E, e->G, s));
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    const int ncu = device_cus();
    int wg = ncu > 0 && ncu < e->TS ? ncu : e->TS;           // one tree slot per workgroup
    // 19x19: MZGO_QUEUE_HELPERS=h gives every searching workgroup h helpers
    // (wg / (1 + h) searches at once, each tree slot's jobs shared)
    if (e->ks->shared_batches) {
      const char* v = getenv("MZGO_QUEUE_HELPERS");
      const int h = v ? atoi(v) : 0;
      if (h > 0 && wg / (1 + h) >= 1) {
        const int leaders = wg / (1 + h);
        sp.helpers = h * leaders;
        wg = leaders * (1 + h);
        HIPCHK(hipMemsetAsync(e->E.jobs, 0, (size_t)leaders * job_bytes(e->A), s));
      }
    }
    HIPCHK(e->ks->search_queue(e->np, sp, pp, e->E, e->G, wg, s));
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    return MZGO_OK;
  }
  if (e->ks->shared_batches) {
    int per = 3;
    if (const char* v = getenv("MZGO_HELPERS_PER_GAME")) per = atoi(v);
    sp.helpers = per > 0 ? per * e->G : 0;
    HIPCHK(hipMemsetAsync(e->E.jobs, 0, (size_t)e->G * job_bytes(e->A), s));
    // the epoch tail: helpers (and workgroups) of ended games join running games
    if (sp.helpers > 0 && sp.factored && pp.moves > 1 && tail_enabled(e->G + sp.helpers)) sp.tail = 1;
  } else if (e->ks->tail_convs && sp.factored && pp.moves > 1 && tail_enabled(e->G)) {
    // the epoch tail (one-strip Winograd boards): a workgroup whose game has
    // ended serves running games' parent convs (records the same either way)
    sp.tail = 1;
    HIPCHK(hipMemsetAsync(e->E.jobs, 0, (size_t)e->G * job_bytes(e->A), s));
  }
  HIPCHK(e->ks->selfplay_move(e->np, np_b, sp, pp, e->E, e->G, s));
  return MZGO_OK;
}

// a launch's PlayParams: the engine's configuration, game generation and test hooks
static PlayParams play_params(const mzgo_engine* e, int arena, int moves) {
  PlayParams pp;
  pp.temperature = e->cfg.temperature;
  pp.temperature_moves = e->cfg.temperature_moves;
  pp.komi = e->cfg.komi;
  pp.game_base = e->cfg.game_base;
  pp.epoch = e->epoch;
  pp.noise = e->noise;
  pp.noise_out = e->noise_out;
  pp.arena = arena;
  pp.moves = moves;
  return pp;
}

}  // extern "C"

// the device replay store's continuous self-play (mzgo_replay_play_games, mzgo_replay.hip)
bool mzgo::engine_noise_hooked(const mzgo_engine* e) { return e->noise != nullptr || e->noise_out != nullptr; }

int mzgo::engine_play_games(mzgo_engine* e, const GamesArgs& ga, hipStream_t s) {
  int rc = e->sync_weights();
  if (rc) return rc;
  const SearchParams sp = e->selfplay_params();        // (no helpers, no tail phase, network 0)
  PlayParams pp = play_params(e, 0, e->M);
  pp.epoch = ga.epoch0;                                // (the kernel derives every game's own epoch from it)
  pp.noise = nullptr;
  pp.noise_out = nullptr;
  const int ncu = device_cus();
  int wg = std::min(ga.n, e->G);                       // workgroup b owns slot b
  if (ncu > 0 && ncu < wg) wg = ncu;
  HIPCHK(hipMemsetAsync(ga.head, 0, sizeof(unsigned), s));
  HIPCHK(hipMemsetAsync(ga.error, 0x7f, sizeof(int), s));
  HIPCHK(e->ks->selfplay_games(e->np, sp, pp, e->E, ga, wg, s));
  e->epoch = ga.epoch0 + (ga.n + e->G - 1) / e->G - 1;
  return MZGO_OK;
}

// the device replay store's window reanalysis (mzgo_replay_reanalyse_sample, mzgo_replay.hip):
// mzgo_reanalyse's schedule, the item count known to the device only (the caller
// has refused board-only and tower engines)
int mzgo::engine_reanalyse_store(mzgo_engine* e, const ReanalyseStoreArgs& ra_arg, int max_items, hipStream_t s) {
  int rc = e->sync_weights();
  if (rc) return rc;
  const SearchParams sp = e->search_params();          // (self-play's row laziness; no helpers, network 0)
  const int ncu = device_cus();
  int wg = ncu > 0 && ncu < e->TS ? ncu : e->TS;       // one tree slot per workgroup
  if (max_items < wg) wg = max_items;
  ReanalyseStoreArgs ra = ra_arg;
  ra.head = e->rq_head;
  HIPCHK(hipMemsetAsync(e->rq_head, 0, sizeof(unsigned), s));
  HIPCHK(e->ks->reanalyse_store(e->np, sp, e->E, ra, wg, s));
  return MZGO_OK;
}

extern "C" {

int mzgo_selfplay_move(mzgo_engine* e, void* stream) { return mzgo_selfplay_moves(e, 1, stream); }

int mzgo_selfplay_set_timing(mzgo_engine* e, int on) {
  if (!e) return fail(MZGO_EINVAL, "bad argument");
  e->timing = on != 0;
  e->tn = 0;
  return MZGO_OK;
}

int mzgo_selfplay_launch_times(mzgo_engine* e, float* boards_ms, float* queue_ms, int cap, int* n_host) {
  if (!e || !n_host || cap < 0 || (cap > 0 && (!boards_ms || !queue_ms))) return fail(MZGO_EINVAL, "bad argument");
  const int n = e->tn < cap ? e->tn : cap;
  for (int i = 0; i < n; ++i) {
    HIPCHK(hipEventSynchronize(e->tev[3 * i + 2]));
    HIPCHK(hipEventElapsedTime(&boards_ms[i], e->tev[3 * i], e->tev[3 * i + 1]));
    HIPCHK(hipEventElapsedTime(&queue_ms[i], e->tev[3 * i + 1], e->tev[3 * i + 2]));
  }
  *n_host = e->tn;
  e->tn = 0;
  return MZGO_OK;
}

int mzgo_selfplay_moves(mzgo_engine* e, int moves, void* stream) {
  if (!e || e->C == 0 || moves < 1) return fail(MZGO_EINVAL, "bad argument");
  int rc = e->sync_weights();
  if (rc) return rc;
  const PlayParams pp = play_params(e, 0, moves);
  if (e->tower) {
    // one move of every game: observation + representation tower + root,
    // S x (select, dynamics tower, expand), action choice + board step
    TowerHost& t = *e->tower;
    hipStream_t s = (hipStream_t)stream;
    const SearchParams sp = e->search_params();
    std::vector<int> st(e->G);
    for (int k = 0; k < moves; ++k) {
      // a tower move is ~43 launches per simulation, so once every game has
      // ended the remaining moves are not enqueued at all: every 4 moves the
      // host reads the slots' status (one small copy per ~4 x S towers)
      if (k > 0 && k % 4 == 0) {
        HIPCHK(hipMemcpyAsync(st.data(), e->E.status, e->G * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (int rc = check_chain(e, s)) return rc;
        bool any = false;
        for (int v : st) any |= v == 0;
        if (!any) break;
      }
      HIPCHK(t.ts->obs(t.TA, sp, pp, e->E, e->G, s));
      HIPCHK(t.root_phase(sp, e->E, e->noise, (long long)e->M * e->A, 1, s));
      HIPCHK(t.simulations(sp, e->E, s));
      HIPCHK(t.ts->choose(t.TA, sp, pp, e->E, e->G, s));
    }
    // (a tower move is ~1.5 s of device work: one synchronisation per call
    // reports an expired chain wait of this call, MZGO_EHIP, and clears it)
    return check_chain(e, s);
  }
  return launch_selfplay(e, e->np, pp, (hipStream_t)stream);
}

int mzgo_arena_move(mzgo_engine* e, mzgo_engine* opponent, void* stream) {
  return mzgo_arena_moves(e, opponent, 1, stream);
}

int mzgo_arena_moves(mzgo_engine* e, mzgo_engine* opponent, int moves, void* stream) {
  if (!e || !opponent || e->C == 0 || moves < 1) return fail(MZGO_EINVAL, "bad argument");
  if (e->tower || opponent->tower) return fail(MZGO_EINVAL, "the arena runs the reference network only (tower 0)");
  if (opponent->N != e->N || opponent->C != e->C)
    return fail(MZGO_EINVAL, "arena engines differ in board size / latent_dim (%d/%d vs %d/%d)", e->N, e->C,
                opponent->N, opponent->C);
  int rc = e->sync_weights();
  if (rc) return rc;
  rc = opponent->sync_weights();
  if (rc) return rc;
  return launch_selfplay(e, opponent->np, play_params(e, 1, moves), (hipStream_t)stream);
}

int mzgo_tower_timing(mzgo_engine* e, int enable, double* tower_ms, int64_t* towers) {
  if (!e || !e->tower) return fail(MZGO_EINVAL, "not a tower engine");
  TowerHost& t = *e->tower;
  HIPCHK(t.harvest());
  if (tower_ms) *tower_ms = t.tower_ms;
  if (towers) *towers = t.towers_timed;
  t.tower_ms = 0.0;
  t.towers_timed = 0;
  t.timing = enable != 0;
  return MZGO_OK;
}

int mzgo_selfplay_inject_noise(mzgo_engine* e, const double* noise) {
  if (!e) return fail(MZGO_EINVAL, "null engine");
  e->noise = noise;
  return MZGO_OK;
}

int mzgo_selfplay_record_noise(mzgo_engine* e, double* dst) {
  if (!e) return fail(MZGO_EINVAL, "null engine");
  if (e->tower) return fail(MZGO_EINVAL, "the noise record covers the reference-network engine (tower 0)");
  e->noise_out = dst;
  return MZGO_OK;
}

int mzgo_tower_record_nodes(mzgo_engine* e, float* dst) {
  if (!e || !e->tower) return fail(MZGO_EINVAL, "not a tower engine");
  e->tower->TA.node_out = dst;
  return MZGO_OK;
}

int mzgo_selfplay_counters(mzgo_engine* e, uint64_t* out, void* stream) {
  if (!e || !out) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long c[kCounters] = {};
  std::vector<int> st(e->G);
  HIPCHK(hipMemcpyAsync(c, e->E.counters, sizeof c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(st.data(), e->E.status, e->G * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (int rc = check_chain(e, s)) return rc;
  int playing = 0;
  for (int v : st) playing += v == 0;
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = (uint64_t)playing; out[4] = c[3]; out[5] = c[4];
  out[6] = c[5]; out[7] = c[6]; out[8] = c[7];
  if (c[8] != 0) {                   // a mzgo_stream_wait_started gate gave up (bounded wait)
    const unsigned long long zero = 0;
    HIPCHK(hipMemcpyAsync(e->E.counters + 8, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return fail(MZGO_EHIP, "mzgo_stream_wait_started: %llu gate(s) gave up before the target count", c[8]);
  }
  return MZGO_OK;
}

int mzgo_search_stats(mzgo_engine* e, uint64_t* out, void* stream) {
  if (!e || !out) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long c[3] = {};
  HIPCHK(hipMemcpyAsync(c, e->E.counters + 9, sizeof c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
  return MZGO_OK;
}

int mzgo_search_stats2(mzgo_engine* e, uint64_t* out, int cap, void* stream) {
  if (!e || !out || cap < 0) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  constexpr int n = kCounters - 9;
  unsigned long long c[n] = {};
  HIPCHK(hipMemcpyAsync(c, e->E.counters + 9, sizeof c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int i = 0; i < (cap < n ? cap : n); ++i) out[i] = c[i];
  return MZGO_OK;
}

int mzgo_records_export(mzgo_engine* e, int g, int32_t* length, int32_t* status, int8_t* stones,
                        uint8_t* invd, uint8_t* flags, int32_t* action, double* value, double* policy,
                        double* reward, double* final_reward, void* stream) {
  if (!e || e->C == 0 || g < 0 || g >= e->G) return fail(MZGO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  int meta[4], st = 0;
  HIPCHK(hipMemcpyAsync(meta, e->E.meta + (size_t)g * 4, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&st, e->E.status + g, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (int rc = check_chain(e, s)) return rc;
  const int L = meta[3];
  if (length) *length = L;
  if (status) *status = st;
  const size_t M = e->M, CELLS = e->CELLS, A = e->A, base = (size_t)g * M;
  if (L > 0) {
    if (stones) HIPCHK(hipMemcpyAsync(stones, e->E.rec_stones + base * CELLS, L * CELLS, hipMemcpyDeviceToHost, s));
    if (invd) HIPCHK(hipMemcpyAsync(invd, e->E.rec_invd + base * CELLS, L * CELLS, hipMemcpyDeviceToHost, s));
    if (flags) HIPCHK(hipMemcpyAsync(flags, e->E.rec_flags + base, L, hipMemcpyDeviceToHost, s));
    if (action) HIPCHK(hipMemcpyAsync(action, e->E.rec_action + base, L * 4, hipMemcpyDeviceToHost, s));
    if (value) HIPCHK(hipMemcpyAsync(value, e->E.rec_value + base, L * 8, hipMemcpyDeviceToHost, s));
    if (policy) HIPCHK(hipMemcpyAsync(policy, e->E.rec_policy + base * A, L * A * 8, hipMemcpyDeviceToHost, s));
    if (reward) HIPCHK(hipMemcpyAsync(reward, e->E.rec_reward + base, L * 8, hipMemcpyDeviceToHost, s));
  }
  if (final_reward) HIPCHK(hipMemcpyAsync(final_reward, e->E.final_reward + g, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return MZGO_OK;
}

#ifdef MZGO_STAMPS
// Diagnostic build only: copy (and zero) the per-slot phase cycle sums.
int mzgo_debug_stamps(mzgo_engine* e, unsigned long long* host) {
  if (!e || !e->E.stamps) return fail(MZGO_EINVAL, "no stamps");
  const size_t n = (size_t)e->TS * kStampPhases;     // every tree slot's row (TS >= G)
  HIPCHK(hipMemcpy(host, e->E.stamps, n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(e->E.stamps, 0, n * 8));
  return MZGO_OK;
}
#endif

// A gate for a collective (mzgo_stream_wait_started, a diagnostic entry
// point): one wave, no LDS and a handful of registers, so it sits beside a
// self-play workgroup on any CU; it returns once *count >= target, or after
// a bounded ~seconds wait, which it records in *expired (reported by the next
// mzgo_selfplay_counters call)
__global__ void __launch_bounds__(64) k_wait_count(const unsigned long long* count, unsigned long long target,
                                                  unsigned long long* expired) {
  if (threadIdx.x != 0) return;
  for (long long spins = 0; spins < (1ll << 26); ++spins) {
    if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
    __builtin_amdgcn_s_sleep(16);
  }
  atomicAdd(expired, 1ull);
}

int mzgo_stream_wait_started(mzgo_engine* e, uint64_t target, void* stream) {
  if (!e || e->C == 0) return fail(MZGO_EINVAL, "bad argument");
  // tower engines run a move as many small launches and never count
  // workgroups_started: the gate would only time out
  if (e->tower) return fail(MZGO_EINVAL, "mzgo_stream_wait_started: not for tower engines");
  hipLaunchKernelGGL(k_wait_count, dim3(1), dim3(64), 0, (hipStream_t)stream, e->E.counters + 6,
                     (unsigned long long)target, e->E.counters + 8);
  HIPCHK(hipGetLastError());
  return MZGO_OK;
}

// Packed records of all G slots, for the multi-GPU gather (layout in mzgo.h).
int mzgo_records_pack(mzgo_engine* e, uint8_t* dst, int64_t capacity, int64_t* bytes_needed, void* stream) {
  if (!e || e->C == 0) return fail(MZGO_EINVAL, "bad argument");
  const size_t G = e->G, M = e->M, CELLS = e->CELLS, A = e->A;
  const size_t sizes[] = {G * M * CELLS, G * M * CELLS, G * M, G * M * 4, G * M * 8, G * M * A * 8,
                          G * M * 8, G * 4 * 4, G * 4, G * 8};
  const void* srcs[] = {e->E.rec_stones, e->E.rec_invd, e->E.rec_flags, e->E.rec_action, e->E.rec_value,
                        e->E.rec_policy, e->E.rec_reward, e->E.meta, e->E.status, e->E.final_reward};
  size_t total = 0;
  for (size_t s : sizes) total += (s + 15) / 16 * 16;
  if (bytes_needed) *bytes_needed = (int64_t)total;
  if (!dst) return MZGO_OK;
  if (capacity < (int64_t)total) return fail(MZGO_EINVAL, "records_pack: buffer of %lld bytes, need %zu", (long long)capacity, total);
  size_t off = 0;
  for (int i = 0; i < 10; ++i) {
    HIPCHK(hipMemcpyAsync(dst + off, srcs[i], sizes[i], hipMemcpyDeviceToDevice, (hipStream_t)stream));
    off += (sizes[i] + 15) / 16 * 16;
  }
  return MZGO_OK;
}

}  // extern "C"
