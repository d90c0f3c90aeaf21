"""Playout cap randomization (KataGo), the parts that need no GPU.

The rule is one host-and-device function (csrc/mzgo_search.hpp
``playout_budget``): a self-play move is searched with ``num_simulations`` when
``fast_simulations`` is 0 or u01(draw(stream_key(seed, key_gid, move), 8, 0)) <
``full_search_prob``, else with ``fast_simulations``.  Here: the host twin, the
engine's refusals, that an all-zero policy row costs the loss nothing, the
host target builder's mask, and the seeds the GPU tests
(tests/test_gpu_playout_cap.py) play with.
"""
import ctypes

import numpy as np
import pytest

# the GPU tests' games: (board, G, S, F, seed, queue games); p = 0.5, game_base 0.  The games are slots
# 0 .. G-1 of epoch 0 and, where the case plays ``play_games_into``, its 2G + 1 queue games (epochs 0 .. 2)
GPU_CASES = {
    "5x5": (5, 4, 25, 8, 3, 0),
    "9x9": (9, 4, 48, 12, 56, 9),
    "19x19": (19, 2, 48, 12, 2, 0),
    "6x6main": (6, 4, 32, 8, 56, 9),
}
GPU_P = 0.5
TAG_BUDGET = 8      # csrc/mzgo_common.hpp; 1-4 are the search's and the weights', 5-7 the replay sampler's


def budgets(seed, key_gid, moves, S, F, p):
    import mzgo
    return [mzgo.playout_budget_host(seed, key_gid, mv, S, F, p) for mv in range(moves)]


def oracle_budget(seed, key_gid, move, S, F, p):
    """The rule restated on oracle/rng.py's counter RNG."""
    from oracle import rng
    if F == 0:
        return S
    h = rng.draw(rng.stream_key(seed, key_gid, move), TAG_BUDGET, 0)
    return S if (h >> 11) * 2.0 ** -53 < p else F


# ---------------------------------------------------------------------------
# 1. the host twin
# ---------------------------------------------------------------------------
def test_host_twin_edges_and_reproducibility():
    import mzgo
    ids = [(g ^ (e << 24), mv) for g in (0, 3, 1000) for e in (0, 1, 200) for mv in (0, 1, 17, 360)]
    for kid, mv in ids:
        assert mzgo.playout_budget_host(9, kid, mv, 200, 0, 0.25) == 200       # off
        assert mzgo.playout_budget_host(9, kid, mv, 200, 0, 0.0) == 200        # off, whatever p
        assert mzgo.playout_budget_host(9, kid, mv, 200, 40, 1.0) == 200       # u01 < 1 always
        assert mzgo.playout_budget_host(9, kid, mv, 200, 40, 0.0) == 40        # u01 < 0 never
        a = mzgo.playout_budget_host(9, kid, mv, 200, 40, 0.25)
        assert a in (200, 40) and a == mzgo.playout_budget_host(9, kid, mv, 200, 40, 0.25)
        assert a == oracle_budget(9, kid, mv, 200, 40, 0.25)
    # the seed, the game and the move each change the draw
    base = [mzgo.playout_budget_host(1, 0, mv, 8, 2, 0.5) for mv in range(64)]
    assert base != [mzgo.playout_budget_host(2, 0, mv, 8, 2, 0.5) for mv in range(64)]
    assert base != [mzgo.playout_budget_host(1, 1, mv, 8, 2, 0.5) for mv in range(64)]
    assert len(set(base)) == 2


def test_host_twin_full_fraction():
    """100,000 (key_gid, move) pairs at p = 0.25: sigma = sqrt(.25 * .75 / 1e5) =
    0.0014, the bound 0.01 is 7 sigma."""
    import mzgo
    full = n = 0
    for e in range(2):
        for g in range(250):
            kid = g ^ (e << 24)
            for mv in range(200):
                full += mzgo.playout_budget_host(1234, kid, mv, 200, 40, 0.25) == 200
                n += 1
    assert n == 100_000
    print("full fraction", full / n)
    assert abs(full / n - 0.25) < 0.01


def test_host_twin_refusals():
    from mzgo._lib import MZGO_EINVAL, lib
    out = ctypes.c_int(-7)
    for args, word in (((1, 0, 0, 8, 9, 0.5), "fast_simulations"), ((1, 0, 0, 8, -1, 0.5), "fast_simulations"),
                       ((1, 0, 0, 8, 2, 1.5), "full_search_prob"), ((1, 0, 0, 8, 2, float("nan")), "full_search_prob"),
                       ((1, 0, -1, 8, 2, 0.5), "move"), ((1, 0, 0, 0, 0, 0.5), "num_simulations")):
        assert lib.mzgo_playout_budget_host(*args, ctypes.byref(out)) == MZGO_EINVAL
        assert word in lib.mzgo_last_error().decode()
    assert lib.mzgo_playout_budget_host(1, 0, 0, 8, 2, 0.5, None) == MZGO_EINVAL
    assert out.value == -7


# ---------------------------------------------------------------------------
# 2. the engine's refusals (all before any device work)
# ---------------------------------------------------------------------------
def _create(**kw):
    from mzgo import EngineConfig
    from mzgo._lib import lib
    c = EngineConfig(**{**dict(board_size=5, latent_dim=96, num_games=1, num_simulations=16), **kw}).to_c()
    h = ctypes.c_void_p()
    rc = lib.mzgo_engine_create(ctypes.byref(c), ctypes.byref(h))
    return rc, lib.mzgo_last_error().decode(), h


@pytest.mark.parametrize("kw,word", [
    (dict(fast_simulations=17), "fast_simulations must be in 0..num_simulations"),
    (dict(fast_simulations=-1), "fast_simulations must be in 0..num_simulations"),
    (dict(fast_simulations=4, full_search_prob=1.25), "full_search_prob must be in [0, 1]"),
    (dict(fast_simulations=4, full_search_prob=-0.01), "full_search_prob must be in [0, 1]"),
    (dict(full_search_prob=float("nan")), "full_search_prob must be in [0, 1]"),
    (dict(latent_dim=64, tower=1, res_blocks=1, fast_simulations=4, full_search_prob=0.5), "tower"),
])
def test_engine_create_refusals(kw, word):
    from mzgo._lib import MZGO_EINVAL
    rc, msg, h = _create(**kw)
    assert rc == MZGO_EINVAL and not h.value
    assert word in msg, msg


def test_defaults_are_off():
    from mzgo import EngineConfig
    from mzgo._lib import Config, lib
    c = Config()
    lib.mzgo_default_config(ctypes.byref(c), 9)
    assert c.fast_simulations == 0 and c.full_search_prob == 1.0
    assert [n for n, _ in Config._fields_][-2:] == ["fast_simulations", "full_search_prob"]
    e = EngineConfig()
    assert e.fast_simulations == 0 and e.full_search_prob == 1.0
    c = EngineConfig(fast_simulations=7, full_search_prob=0.25).to_c()
    assert c.fast_simulations == 7 and c.full_search_prob == 0.25


# ---------------------------------------------------------------------------
# 3. an all-zero policy row costs nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("transform", [True, False])
def test_zero_policy_rows_cost_nothing(transform):
    import mzgo
    B, K, A = 5, 3, 26
    rs = np.random.RandomState(5)
    logits = (rs.randn(K + 1, B, A) * 3).astype(np.float32)
    value = rs.randn(K + 1, B).astype(np.float32)
    reward = rs.randn(K, B).astype(np.float32)
    t_pol = rs.rand(B, K + 1, A).astype(np.float32)
    t_pol /= t_pol.sum(-1, keepdims=True)
    t_val = rs.randn(B, K + 1).astype(np.float32)
    t_rew = rs.randint(-1, 2, (B, K)).astype(np.float32)
    masked = [(0, 0), (0, 3), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3)]       # (sample, step); sample 4 entirely
    kw = dict(value_loss_weight=1.0, policy_loss_weight=1.0, reward_loss_weight=1.0, value_transform=transform)
    full = mzgo.unroll_loss_host(logits, value, reward, t_pol, t_val, t_rew, **kw)
    zp = t_pol.copy()
    for b, k in masked:
        zp[b, k] = 0.0
    got = mzgo.unroll_loss_host(logits, value, reward, zp, t_val, t_rew, **kw)
    keep = np.ones((K + 1, B), bool)
    for b, k in masked:
        keep[k, b] = False
        assert not got[2][k, b].any(), (b, k)                  # g_logits exactly 0
    # every other row's gradient bits, and the value / reward gradients, are the unmasked call's
    np.testing.assert_array_equal(got[2][keep].view(np.uint32), full[2][keep].view(np.uint32))
    np.testing.assert_array_equal(got[3].view(np.uint32), full[3].view(np.uint32))
    np.testing.assert_array_equal(got[4].view(np.uint32), full[4].view(np.uint32))
    # the value and reward totals do not move; samples without a masked row keep their loss bits
    assert got[1][1] == full[1][1] and got[1][3] == full[1][3]
    np.testing.assert_array_equal(got[0][[1, 3]].view(np.uint32), full[0][[1, 3]].view(np.uint32))
    # a batch of masked rows alone: policy loss exactly 0
    only = mzgo.unroll_loss_host(logits, value, reward, np.zeros_like(t_pol), t_val, t_rew, **kw)
    assert only[1][2] == 0.0 and not only[2].any()
    # ... and sample 4, all of whose rows are masked, has exactly its value + reward loss
    solo = mzgo.unroll_loss_host(logits[:, 4:5], value[:, 4:5], reward[:, 4:5], np.zeros((1, K + 1, A), np.float32),
                                 t_val[4:5], t_rew[4:5], **kw)
    assert solo[1][2] == 0.0
    assert got[0][4] == solo[0][0]


# ---------------------------------------------------------------------------
# 4. the host target builder
# ---------------------------------------------------------------------------
def test_host_builder_masks_fast_rows():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    N, K = 5, 3
    A = N * N + 1
    trajs = synthetic_trajectories(N, 4, seed=9)
    net = mzgo.MuZeroNet(32, A)
    net.load_state_dict(mzgo.deterministic_state_dict(32, A, 3))
    tr = MuZeroTrainer(net, TrainConfig(unroll_steps=K), mode="batched")
    rs = np.random.RandomState(2)
    fast = [list(rs.rand(len(t["actions"])) < 0.5) for t in trajs]
    fast[3] = [False] * len(fast[3])                       # a game without one
    assert all(any(f) and not all(f) for f in fast[:3])
    capped = [dict(t, fast_search=f) for t, f in zip(trajs, fast)]
    starts = [0, len(trajs[1]["actions"]) - 1, len(trajs[2]["actions"]) // 2, 1]
    plain = tr.batch_targets(trajs, starts)
    got = tr.batch_targets(capped, starts)
    for a, b in zip(got[:4], plain[:4]):                   # obs0, acts, t_val, t_rew: unchanged
        np.testing.assert_array_equal(a, b)
    seen_zero = seen_kept = seen_past = 0
    for b, (t, s) in enumerate(zip(capped, starts)):
        T = len(t["actions"])
        for k in range(K + 1):
            i = s + k
            if i < T and t["fast_search"][i]:
                assert not got[4][b, k].any()
                seen_zero += 1
            else:
                np.testing.assert_array_equal(got[4][b, k].view(np.uint64), plain[4][b, k].view(np.uint64))
                seen_kept += i < T
                seen_past += i >= T
    assert seen_zero and seen_kept and seen_past           # (past the end: the uniform row stays)
    # reference mode reads the same rule
    ref = MuZeroTrainer(net, TrainConfig(unroll_steps=K), mode="reference")
    i = fast[0].index(True)
    assert not ref._policy_target(capped[0], i).any()
    assert ref._policy_target(trajs[0], i) is trajs[0]["policies"][i]


def test_trajectory_from_record_names_fast_moves_only_when_there_are_some():
    from mzgo.selfplay import history_from_device
    from mzgo.trainer import trajectory_from_record
    N, L = 5, 4
    A = N * N + 1
    rec = dict(length=L, status=1, stones=np.zeros((L, N * N), np.int8), invd=np.zeros((L, N * N), np.uint8),
               flags=np.array([0, 1, 0, 1], np.uint8), action=np.array([0, 1, 2, 3], np.int32),
               value=np.zeros(L), policy=np.full((L, A), 1.0 / A), reward=np.zeros(L), final_reward=0.0)
    final = np.zeros((6, N, N))
    t = trajectory_from_record(rec, final, N, 40)
    assert "fast_search" not in t
    assert history_from_device(rec, N, 0.99).fast_search == [False] * L
    rec["flags"] = np.array([0, 1 | 8, 8, 1], np.uint8)
    t = trajectory_from_record(rec, final, N, 40)
    assert t["fast_search"] == [False, True, True, False]
    assert [o[2].max() for o in t["observations"][:L]] == [0, 1, 0, 1]       # bit 3 is no plane
    h = history_from_device(rec, N, 0.99)
    assert h.fast_search == [False, True, True, False]
    assert "fast_search" not in h.to_record()                                # the reference's pickle format stays


# ---------------------------------------------------------------------------
# 5. the GPU tests' seeds give both kinds of move
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_gpu_seeds_give_fast_and_full_moves(case):
    from mzgo.replay import queue_key_gids
    N, G, S, F, seed, queued = GPU_CASES[case]
    assert queued in (0, 2 * G + 1)
    kids = {int(g) for g in range(G)} | {int(k) & 0xFFFFFFFF for k in queue_key_gids(queued, G, 0, 0)}
    for kid in sorted(kids):
        b = budgets(seed, kid, 12, S, F, GPU_P)
        assert b.count(F) >= 5 and b.count(S) >= 5, (case, kid, b)
