"""GPU: reanalysis (mzgo_reanalyse / k_reanalyse_queue) -- stored positions
searched from one device work queue.

Engines here are small (num_games = 4 tree slots, compat "fixed" so that a
19x19 engine keeps 4 slots too -- compat plays no part in a search), so a
list of n > 4 positions makes every workgroup claim several items.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAIN = dict(c_puct=2.0, dirichlet_alpha=0.03, dirichlet_epsilon=0.25, pass_epsilon=0.05, search_variant="main")


@functools.lru_cache(maxsize=None)
def _net(N, C=96):
    import mzgo
    from oracle.weights import deterministic_state_dict
    net = mzgo.MuZeroNet(C, N * N + 1).to("cuda").eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state_dict(C, N * N + 1, 0).items()})
    return net


@functools.lru_cache(maxsize=None)
def _positions(N, n, seed):
    """n random mid-game observations f64 [n, 6, N, N] (shared, read-only)."""
    from oracle.positions import random_position
    obs = np.stack([random_position(N, 3 + (5 * i) % (N * N // 2), seed + i) for i in range(n)])
    obs.setflags(write=False)
    return obs


def _valid_mask(invd, pass_epsilon):
    """self_play.py:152-158's valid_mask for records' INVD planes [L, N*N]: 1 on
    legal cells, and on the pass pass_epsilon while a cell is legal, else 1."""
    cells = (invd == 0).astype(np.float64)
    return np.concatenate([cells, np.where(cells.any(1), pass_epsilon, 1.0)[:, None]], axis=1)


def _reanalyse(eng, obs, ids, noise=None, want_policy=True):
    from mzgo.reanalyse import positions_from_planes
    stones, invd, flags = positions_from_planes(obs)
    vis, val, pol = eng.reanalyse(stones, invd, flags, np.asarray(ids, np.int32), noise=noise,
                                  want_policy=want_policy)
    return vis.cpu().numpy(), val.cpu().numpy(), (pol.cpu().numpy() if pol is not None else None)


# ---------------------------------------------------------------------------
# 1. against the reference's own trees
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["5x5_s25_empty", "5x5_s25_mid", "9x9_s200_mid", "19x19_s800_mid"])
def test_queue_search_matches_reference_tree(golden_dir, case):
    """A queue search returns the visit counts of the tree recorded from the
    reference MCTS.run (the fixture test_gpu_search.py checks mzgo_search
    against), from item 2 of a 6-item list on 4 slots."""
    from oracle.rng import injected_noise
    g = np.load(f"{golden_dir}/mcts_{case}.npz")
    N, S = int(g["N"]), int(g["S"])
    seed, game, move = int(g["seed"]), int(g["game"]), int(g["move"])
    A = N * N + 1
    eng = _net(N).engine(num_games=4, num_simulations=S, seed=seed, compat="fixed")
    obs = np.array(_positions(N, 6, 900))
    ids = np.array([[50 + i, i] for i in range(6)], np.int32)
    noise = np.stack([injected_noise(seed, 50 + i, i, A) for i in range(6)])
    obs[2], ids[2], noise[2] = g["obs"], (game, move), injected_noise(seed, game, move, A)
    vis, val, _ = _reanalyse(eng, obs, ids, noise=noise)
    np.testing.assert_array_equal(vis[2], g["visits"])
    assert abs(val[2] - float(g["root_value"])) < 1e-5


# ---------------------------------------------------------------------------
# 2. equals mzgo_search
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", [(5, 25), (9, 64), (9, 600), (19, 100)])
def test_reanalyse_equals_search(N, S):
    """11 positions through the 4-slot queue == an 11-slot mzgo_search launch
    (sampled noise, the same keys); 9x9 / 600 runs the HBM tree."""
    n = 11
    net = _net(N)
    obs = _positions(N, n, 40)
    wide = net.engine(num_games=n, num_simulations=S, seed=5, compat="fixed")
    vis_s, val_s = wide.search(torch.from_numpy(obs.copy()), move_index=3)
    eng = net.engine(num_games=4, num_simulations=S, seed=5, compat="fixed")
    vis, val, _ = _reanalyse(eng, obs, [(i, 3) for i in range(n)], want_policy=False)
    np.testing.assert_array_equal(vis, vis_s.cpu().numpy())
    np.testing.assert_array_equal(val, val_s.cpu().numpy())


# ---------------------------------------------------------------------------
# 3. reproduces self-play records, compat "reference" (the move-parallel epoch)
# ---------------------------------------------------------------------------
def _same_records(a, b):
    for ra, rb in zip(a, b):
        assert ra["length"] == rb["length"] and ra["status"] == rb["status"]
        assert ra["final_reward"] == rb["final_reward"]
        for k in ("stones", "invd", "flags", "action", "value", "policy", "reward"):
            assert ra[k].tobytes() == rb[k].tobytes(), k


@pytest.mark.parametrize("epoch", [0, 1])
@pytest.mark.parametrize("N,G,S,max_moves", [(9, 8, 32, 0), (19, 2, 48, 12)])
def test_reanalyse_reproduces_move_parallel_records(N, G, S, max_moves, epoch):
    """Every (game, move) search of a whole-game move-parallel launch, run
    again through the reanalysis queue with the record's key, gives the
    recorded root value to the byte; the records are left as they were."""
    import mzgo
    sp = mzgo.SelfPlay(_net(N), G, S, seed=77, max_moves=max_moves)
    sp.reset(epoch)
    sp.move(sp.max_moves)
    eng = sp.engine
    assert eng.counters()["playing"] == 0
    before = [eng.record(g) for g in range(G)]
    out = sp.reanalyse()
    after = [eng.record(g) for g in range(G)]
    _same_records(before, after)
    assert sum(r["length"] for r in before) > G
    for rec, (vis, val, pol) in zip(before, out):
        L = rec["length"]
        assert vis.shape == (L, N * N + 1) and pol.shape == (L, N * N + 1)
        assert val.tobytes() == rec["value"].tobytes()
        # the policy a compat "reference" record lacks: visit_counts * valid_mask / sum
        # (f64 sums of <= 362 terms in another order: within 362 * 2^-53 < 1e-13 relative)
        vm = vis * _valid_mask(rec["invd"], eng.config.pass_epsilon)
        assert (vm.sum(1) > 0).all()
        np.testing.assert_allclose(pol, vm / vm.sum(1, keepdims=True), rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------
# 4. policy equals compat "fixed" records
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["self_play", "main"])
@pytest.mark.parametrize("N,S", [(5, 25), (9, 48)])
def test_policy_equals_fixed_records(N, S, variant):
    import mzgo
    G = 4
    opts = dict(MAIN) if variant == "main" else {}
    sp = mzgo.SelfPlay(_net(N), G, S, seed=31, compat="fixed", **opts)
    sp.reset()
    sp.move(sp.max_moves)
    eng = sp.engine
    assert eng.counters()["playing"] == 0
    recs = [eng.record(g) for g in range(G)]
    out = sp.reanalyse()
    checked = 0
    for rec, (vis, val, pol) in zip(recs, out):
        L = rec["length"]
        assert pol.tobytes() == rec["policy"].tobytes()
        assert val.tobytes() == rec["value"].tobytes()
        mask = _valid_mask(rec["invd"], eng.config.pass_epsilon)
        # the move rule is the argmax (first max) of the masked counts: main.py's
        # always (counts where the mask is > 0), self_play.py's (counts * mask)
        # once the temperature is 0 (move >= temperature_moves)
        vm = vis * (mask > 0) if variant == "main" else vis * mask
        rule = vm.sum(1) > 0
        if variant == "self_play":
            rule &= np.arange(L) >= eng.config.temperature_moves
        np.testing.assert_array_equal(vm.argmax(1)[rule], rec["action"][rule])
        checked += int(rule.sum())
    assert checked > 0


# ---------------------------------------------------------------------------
# 5. queue mechanics
# ---------------------------------------------------------------------------
QN, QS = 9, 32


@functools.lru_cache(maxsize=None)
def _queue_reference():
    """13 = 3 * TS + 1 items on 4 slots; items 0, 5, 9, 12 are one position and id."""
    n = 13
    obs = np.array(_positions(QN, n, 500))
    ids = np.array([[7 + i, 2 * i] for i in range(n)], np.int32)
    for j in (5, 9, 12):
        obs[j], ids[j] = obs[0], ids[0]
    eng = _net(QN).engine(num_games=4, num_simulations=QS, seed=3, compat="fixed")
    out = _reanalyse(eng, obs, ids)
    for a in (obs, ids, *out):
        a.setflags(write=False)
    return obs, ids, out


def test_queue_single_item():
    obs, ids, (vis, val, pol) = _queue_reference()
    eng = _net(QN).engine(num_games=4, num_simulations=QS, seed=3, compat="fixed")
    v1, x1, p1 = _reanalyse(eng, obs[3:4], ids[3:4])
    np.testing.assert_array_equal(v1[0], vis[3])
    assert x1[0] == val[3]
    np.testing.assert_array_equal(p1[0], pol[3])
    assert v1.sum() > 0 and abs(p1.sum() - 1.0) < 1e-12


def test_queue_repeated_item_gives_identical_rows():
    _, _, (vis, val, pol) = _queue_reference()
    for j in (5, 9, 12):
        np.testing.assert_array_equal(vis[j], vis[0])
        assert val[j] == val[0]
        np.testing.assert_array_equal(pol[j], pol[0])
    assert len({v.tobytes() for v in vis}) == 10          # the other rows are their own searches


def test_queue_permuted_list_gives_permuted_rows():
    obs, ids, ref = _queue_reference()
    perm = np.random.default_rng(0).permutation(len(ids))
    eng = _net(QN).engine(num_games=4, num_simulations=QS, seed=3, compat="fixed")
    got = _reanalyse(eng, obs[perm], ids[perm])
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b[perm])


def test_queue_result_does_not_depend_on_slot_count():
    obs, ids, ref = _queue_reference()
    for G in (2, 8):
        eng = _net(QN).engine(num_games=G, num_simulations=QS, seed=3, compat="fixed")
        got = _reanalyse(eng, obs, ids)
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def _raw_call(eng, n):
    from mzgo._lib import lib, ptr, stream_of
    A, cells = eng.A, eng.N * eng.N
    dev = eng.device
    m = max(n, 1)
    stones = torch.zeros(m, cells, dtype=torch.int8, device=dev)
    invd = torch.zeros(m, cells, dtype=torch.uint8, device=dev)
    flags = torch.zeros(m, dtype=torch.uint8, device=dev)
    ids = torch.zeros(m, 2, dtype=torch.int32, device=dev)
    vis = torch.zeros(m, A, dtype=torch.int32, device=dev)
    val = torch.zeros(m, dtype=torch.float64, device=dev)
    rc = lib.mzgo_reanalyse(eng.handle, ptr(stones), ptr(invd), ptr(flags), ptr(ids), None, n, ptr(vis), ptr(val),
                            None, stream_of(dev))
    torch.cuda.synchronize()
    return rc, lib.mzgo_last_error().decode()


def test_refusals():
    from mzgo import Engine, EngineConfig
    from mzgo._lib import MZGO_EINVAL, MZGO_ENOWEIGHTS, MZGO_OK, lib
    good = _net(5).engine(num_games=4, num_simulations=8, compat="fixed")
    assert _raw_call(good, 2)[0] == MZGO_OK
    rc, msg = _raw_call(good, 0)
    assert rc == MZGO_EINVAL and msg
    rc = lib.mzgo_reanalyse(None, None, None, None, None, None, 1, None, None, None, None)
    assert rc == MZGO_EINVAL and lib.mzgo_last_error()
    for cfg, want in ((EngineConfig(board_size=5, latent_dim=0, num_games=2), MZGO_EINVAL),
                      (EngineConfig(board_size=5, latent_dim=64, num_games=2, num_simulations=4, tower=1,
                                    res_blocks=1), MZGO_EINVAL),
                      (EngineConfig(board_size=5, num_games=2, num_simulations=4), MZGO_ENOWEIGHTS)):
        eng = Engine(cfg)
        rc, msg = _raw_call(eng, 2)
        assert rc == want, (cfg, rc, msg)
        assert msg
        eng.close()


# ---------------------------------------------------------------------------
# 7. trainer level
# ---------------------------------------------------------------------------
def test_reanalyser_reproduces_then_refreshes_main_trajectories():
    import mzgo
    from mzgo.reanalyse import Reanalyser, record_ids
    from mzgo.trainer import MainSelfPlay
    from oracle.weights import deterministic_state_dict
    N, S, G, seed = 5, 16, 4, 13
    A = N * N + 1
    net = mzgo.MuZeroNet(96, A).to("cuda").eval()         # (its own net: the test changes the weights)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state_dict(96, A, 0).items()})
    trajs = MainSelfPlay(net, G, S, seed=seed).play()
    ids = [record_ids(0, g, 0, np.arange(len(t["actions"]))) for g, t in enumerate(trajs)]
    ra = Reanalyser(net, S, slots=4, seed=seed)
    same = ra.run(trajs, ids)
    for t0, t1 in zip(trajs, same):
        assert len(t1["policies"]) == len(t0["policies"]) == len(t1["root_values"]) == len(t0["actions"])
        np.testing.assert_array_equal(np.array(t1["policies"]), np.array(t0["policies"]))
        assert t1["actions"] == t0["actions"] and t1["rewards"] == t0["rewards"]
    gen = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(p.device))
    ra.refresh(net)
    fresh = ra.run(trajs, ids)
    differs = False
    for t0, t1 in zip(trajs, fresh):
        for o, p0, p1 in zip(t0["observations"], t0["policies"], t1["policies"]):
            assert abs(p1.sum() - 1.0) < 1e-12
            assert not p1[:N * N][o[3].reshape(-1) > 0].any()
            differs |= not np.array_equal(p0, p1)
    assert differs
