"""Position-level prioritized replay on the GPU (mzgo.DeviceReplay
``enable_position_priorities`` / ``sample_positions*`` /
``update_position_priorities``; csrc/mzgo_replay.hip: k_replay_new_positions,
k_replay_possample_build, k_replay_possample_draw,
k_replay_update_position_priorities) and ``TrainConfig.position_priorities``.

The sampler's kernels are compared bit for bit with the host twin, which
tests/test_replay_positions.py compares with an independent restatement; the
stores are 5x5 boards with ``max_moves`` 130 whose games (of 0 .. 130 moves,
test_replay_positions.build_pos_case) come from synthetic host trajectories
through ``add``.  The weights of new games are compared with the td rule's
host twin on the exported games.
"""
import functools

import numpy as np
import pytest
import torch

from test_replay_positions import FLT_MIN, M, build_pos_case

pytestmark = pytest.mark.gpu

N, A = 5, 26
DISCOUNT = 0.99


def _np(t):
    return t.cpu().numpy()


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _planes(n):
    """n + 1 5x5 'positions' (what they show does not matter to the sampler)."""
    obs = []
    for t in range(n + 1):
        o = np.zeros((6, N, N))
        o[t % 2].flat[t % (N * N)] = 1.0
        o[2] = t % 2
        obs.append(o)
    return obs


def _game(T, k):
    """A 5x5 'game' of T moves in main.py's format with rewards and root values."""
    r = np.random.default_rng(1000 + k)
    obs = _planes(M)[:T + 1]
    return dict(observations=obs + [obs[-1]], actions=[(t + k) % A for t in range(T)],
                rewards=[float(x) for x in r.uniform(-1, 1, T)] + [1.0], policies=[np.full(A, 1.0 / A)] * T,
                root_values=[float(x) for x in r.uniform(-1, 1, T)])


@functools.lru_cache(maxsize=None)
def _store(cap, wrap=True):
    """A store whose slots hold build_pos_case(cap): cap + head adds (game k
    lands in slot k % cap: the ring ends wrapped at ``head``), or with
    ``wrap=False`` cap adds (head 0); then the case's position weights."""
    import mzgo
    pprio, length, head = build_pos_case(cap)
    head = head if wrap else 0
    rp = mzgo.DeviceReplay(N, cap, M, "cuda")
    rp.enable_position_priorities(3, DISCOUNT, init="uniform")
    for k in range(cap + head):
        rp.add(_game(int(length[k % cap]), k))
    assert len(rp) == cap
    rp.set_position_priorities(pprio[(head + np.arange(cap)) % cap])
    return rp, head


def _assert_sampler_equals_twin(cap, wrap, draws):
    from mzgo.replay import sample_positions_host
    pprio, length, _ = build_pos_case(cap)
    rp, head = _store(cap, wrap)
    order = (head + np.arange(cap)) % cap
    got_w = _np(rp.position_priorities())
    for i, slot in enumerate(order):
        np.testing.assert_array_equal(_u64(got_w[i, :length[slot]]), _u64(pprio[slot, :length[slot]]))
    want_gen = 1 + (np.arange(cap) < head)
    for B, sym, beta in draws:
        step = 10 * cap + B
        got = rp.sample_positions(B, seed=21, step=step, symmetries=sym, beta=beta)
        want = sample_positions_host(pprio, length, head, B, seed=21, step=step, symmetries=sym, beta=beta)
        np.testing.assert_array_equal(_np(got["items"]), want["items"])
        np.testing.assert_array_equal(_np(got["index"]), want["index"])
        np.testing.assert_array_equal(_np(got["gen"]), want_gen[want["items"][:, 0]])
        np.testing.assert_array_equal(_np(got["weight"]).view(np.uint32), want["weight"].view(np.uint32))
        assert _np(got["weight"]).max() == 1.0
        again = rp.sample_positions(B, seed=21, step=step, symmetries=sym, beta=beta)
        for k in ("index", "items", "gen", "weight"):
            assert torch.equal(got[k], again[k]), k
        mine = rp.sample_positions_host(B, seed=21, step=step, symmetries=sym, beta=beta)
        np.testing.assert_array_equal(mine["items"], want["items"])
        slots, starts = want["items"][:, 0], want["items"][:, 1]
        assert len(set(slots.tolist())) == B and (pprio[slots, starts] > 0).all() and (starts < length[slots]).all()


@pytest.mark.parametrize("cap", [1, 63, 64, 65, 130])
def test_kernel_equals_the_twin(cap):
    _, length, _ = build_pos_case(cap)
    n_valid = int((length > 0).sum())
    _assert_sampler_equals_twin(cap, True, ((1, False, 0.0), (min(n_valid, 7), True, 0.5), (n_valid, True, 1.0)))


def test_kernel_equals_the_twin_at_4097_slots():
    _, length, _ = build_pos_case(4097)
    n_valid = int((length > 0).sum())
    assert n_valid > 128
    _assert_sampler_equals_twin(4097, False, ((128, True, 0.5),))


def test_one_move_games_draw_as_the_game_sampler():
    """Both samplers' kernels descend one tree: where every game has one move
    and pprio[game][0] = prio[game], ``sample_positions`` returns ``sample``'s
    items, index, gen and weight byte for byte (test_replay_positions has the
    reasons and the host twins' side).  65 slots: two level-1 groups, the second
    of one slot; the ring wrapped, six games without a move; all the others drawn."""
    import mzgo
    cap, head = 65, 20
    rp = mzgo.DeviceReplay(N, cap, 2, "cuda")
    rp.enable_position_priorities(1, DISCOUNT, init="uniform")
    for k in range(cap + head):
        rp.add(_game(int(k % 11 != 3), k))
    r = np.random.default_rng(65)
    prio = 10.0 ** r.uniform(-34.0, 1.0, cap)
    rp.set_device_priorities(prio)
    rp.set_position_priorities(np.stack([prio, 10.0 ** r.uniform(-34.0, 1.0, cap)], axis=1))   # (column 1: never read)
    B = int((np.asarray(rp.lengths) > 0).sum())
    assert B == cap - 6
    draw = dict(seed=21, step=7, symmetries=True, beta=0.5)
    want, got = rp.sample(B, **draw), rp.sample_positions(B, **draw)
    for k in ("items", "index", "gen", "weight"):
        assert _np(got[k]).tobytes() == _np(want[k]).tobytes(), k
    items = _np(want["items"])
    np.testing.assert_array_equal(items, rp.sample_host(B, **draw)["items"])
    assert len(set(items[:, 0].tolist())) == B and (items[:, 1] == 0).all() and len(set(items[:, 2].tolist())) > 1
    assert set(_np(want["gen"]).tolist()) == {1, 2} and 0 < _np(want["weight"]).min() < 1.0
    rp.close()


# ---------------------------------------------------------------------------
# new games
# ---------------------------------------------------------------------------
def _assert_td_weights(rp, td, alpha, floor=None):
    """position_priorities() against the host rule on the exported games."""
    from mzgo.replay import position_priorities_host
    got = _np(rp.position_priorities())
    assert got.shape == (len(rp), rp.max_moves)
    moves = 0
    for i in range(len(rp)):
        g = rp.export(i)
        L = len(g["actions"])
        want = position_priorities_host(g["rewards"], g["root_values"], td, DISCOUNT, alpha, floor)
        if alpha == 1.0:
            np.testing.assert_array_equal(_u64(got[i, :L]), _u64(want), err_msg=f"game {i}")
        else:                                              # (the device's pow: a few ulp from the C library's)
            np.testing.assert_allclose(got[i, :L], want, rtol=1e-14, err_msg=f"game {i}")
        moves += L
    return moves


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_new_games_get_the_td_rule(alpha):
    import mzgo
    from mzgo.trainer import MainSelfPlay
    from test_gpu_replay import _net
    G, td = 4, 3
    msp = MainSelfPlay(_net(N, 96, 5).eval(), G, 8, seed=3)
    rp = mzgo.DeviceReplay(N, 10, msp.max_moves, "cuda")
    msp.play_into(rp)                                                   # add_games, before the ledger exists
    rp.enable_position_priorities(td, DISCOUNT, alpha=alpha)           # ... fills the games held
    rp.enable_position_priorities(td, DISCOUNT, alpha=alpha)           # (the same again: a no-op)
    assert _assert_td_weights(rp, td, alpha) > 0
    np.testing.assert_array_equal(_np(rp.device_priorities()), [1.0] * 4)
    msp.play_into(rp)                                                   # add_games with the ledger: slots 4..7
    rp.add(_game(7, 1))                                                 # slot 8
    assert len(rp) == 9 and _assert_td_weights(rp, td, alpha) > 7
    rp.set_device_priorities(np.arange(2.0, 11.0))
    msp.play_games_into(rp, 2 * G)                                      # slots 9, then 0..6 again: wrapped
    assert len(rp) == 10
    _assert_td_weights(rp, td, alpha)
    # the game-level ledger is what it is without the position ledger
    np.testing.assert_array_equal(_np(rp.device_priorities()), [9.0, 10.0] + [1.0] * 8)
    np.testing.assert_array_equal(_np(rp.device_generations()), [1, 1, 1] + [2] * 7)
    # a uniform store
    ru = mzgo.DeviceReplay(N, 3, 12, "cuda")
    ru.enable_position_priorities(td, DISCOUNT, init="uniform")
    for k, T in enumerate((5, 0, 12, 1)):
        ru.add(_game(T, k))
    got = _np(ru.position_priorities())
    for i, T in enumerate((0, 12, 1)):
        np.testing.assert_array_equal(got[i, :T], np.ones(T))


# ---------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------
def _small(alpha=1.0, floor=None, lengths=(5, 2, 9, 4)):
    import mzgo
    rp = mzgo.DeviceReplay(N, len(lengths), 12, "cuda")
    rp.enable_position_priorities(3, DISCOUNT, alpha=alpha, floor=floor, init="uniform")
    for k, T in enumerate(lengths):
        rp.add(_game(T, k))
    return rp


@pytest.mark.parametrize("alpha,floor", [(1.0, None), (1.0, 0.25), (0.5, 0.25)])
def test_position_priority_update(alpha, floor):
    K, lengths = 3, (5, 2, 9, 4)
    rp = _small(alpha, floor, lengths)
    B = len(lengths)
    s = rp.sample_positions(B, seed=4, step=1)
    items = _np(s["items"])
    r = np.random.default_rng(5)
    value = r.uniform(-1, 1, (B, K + 1)).astype(np.float32)
    t_val = r.uniform(-1, 1, (B, K + 1)).astype(np.float32)
    t_val[1, 0] = value[1, 0]                                           # an error of 0: the floor
    value[0, 0] = np.nan                                                # (row ``start`` is always inside the game)
    t_val[2, 0] = np.inf
    rp.update_position_priorities(s, torch.from_numpy(value).cuda(), torch.from_numpy(t_val).cuda())
    fl = FLT_MIN if floor is None else floor
    want = np.ones((B, 12))
    written = 0
    for b, (slot, start, _) in enumerate(items):                        # (slot = logical index here)
        for k in range(K + 1):
            err = abs(np.float64(value[b, k]) - np.float64(t_val[b, k]))
            if start + k < lengths[slot] and np.isfinite(err):
                want[slot, start + k] = max(err, fl) ** alpha
                written += 1
    got = _np(rp.position_priorities())
    assert 0 < written < B * (K + 1) - 2                                # some rows lie past a game's end
    for i, L in enumerate(lengths):
        if alpha == 1.0:
            np.testing.assert_array_equal(_u64(got[i, :L]), _u64(want[i, :L]))
        else:
            np.testing.assert_allclose(got[i, :L], want[i, :L], rtol=1e-14)
    assert abs(got[items[1, 0], items[1, 1]] - fl ** alpha) <= (0.0 if alpha == 1.0 else 1e-14 * fl ** alpha)
    assert rp.skipped_updates() == 2                                    # the NaN and the inf, each counted, weights kept
    np.testing.assert_array_equal(_np(rp.device_priorities()), [1.0] * B)          # the game-level weights: untouched


def test_generation_guard():
    K, lengths = 3, (5, 2, 9, 4)
    rp = _small(lengths=lengths)
    s = rp.sample_positions(4, seed=2, step=0)
    items = _np(s["items"])
    rp.add(_game(6, 50))                                                # evicts logical 0 = slot 0
    value = torch.full((4, K + 1), 3.0, device="cuda")
    rp.update_position_priorities(s, value, torch.zeros_like(value))
    got = _np(rp.position_priorities())                                 # logical i is slot (1 + i) % 4
    np.testing.assert_array_equal(got[3, :6], np.ones(6))               # the fresh game keeps its fresh weights
    for slot, start, _ in items:
        if slot != 0:
            L = lengths[slot]
            want = np.ones(L)
            want[start:start + K + 1] = 3.0
            np.testing.assert_array_equal(got[slot - 1, :L], want)
    assert rp.skipped_updates() == 0


# ---------------------------------------------------------------------------
# the items feed the rest of the pipeline unchanged
# ---------------------------------------------------------------------------
def test_items_go_through_the_assembly_and_the_window_reanalysis():
    from test_gpu_reanalyse_sample import GID0, _reanalyser, _rows
    from test_gpu_replay import _assert_same_bits, _net, _store as game_store
    from test_gpu_value_targets import _valued
    trajs = _valued()
    B, K, n = len(trajs), 3, 4
    rp = game_store(N, trajs, gid0=GID0)
    rp.enable_position_priorities(n, DISCOUNT)
    for step in range(2):
        draw = dict(seed=8, step=step, symmetries=True, beta=0.5)
        s = rp.sample_positions(B, **draw)
        host = rp.sample_positions_host(B, **draw)
        items = _np(s["items"])
        np.testing.assert_array_equal(items, host["items"])
        idx, starts, syms = _np(s["index"]), items[:, 1], items[:, 2]
        assert sorted(idx.tolist()) == list(range(B))
        want = rp.batch(idx, starts, K, DISCOUNT, syms)
        for got in (rp.batch_from(s, K, DISCOUNT), rp.sample_positions_batch(B, K, DISCOUNT, **draw)):
            for name, w in want.items():
                _assert_same_bits(got[name], w, name)
        want_v = rp.batch_values(idx, starts, K, n, DISCOUNT, syms)
        both = rp.sample_positions_batch_values(B, K, n, DISCOUNT, **draw)
        for got in (rp.batch_values_from(s, K, n, DISCOUNT), both):
            for name, w in want_v.items():
                _assert_same_bits(got[name], w, name)
        for name in ("items", "index", "gen", "weight"):
            _assert_same_bits(both[name], s[name], name)
    assert len(set(starts.tolist())) > 1 and syms.max() > 0
    # the window reanalysis searches exactly the rows the items list
    net = _net(N, 96, 0).eval()
    weights = _np(rp.position_priorities())
    before = _rows(rp)
    listed = rp.window_items_host(s, K)
    count = rp.reanalyse_sample(_reanalyser(net), s, K)
    assert count.item() == len(listed) > 0
    after = _rows(rp)
    inside = {(int(a), int(b)) for a, b in listed}
    for k in range(B):
        for row in range(len(trajs[k]["actions"])):
            changed = not np.array_equal(after[k][0][row], before[k][0][row]) or after[k][1][row] != before[k][1][row]
            assert changed == ((k, row) in inside), (k, row)
    np.testing.assert_array_equal(_u64(_np(rp.position_priorities())), _u64(weights))      # (not refreshed by a search)


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
def _run(fused, C, target, position, ledger, steps=3):
    """``steps`` train steps on a fresh store and net; what they leave behind."""
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from test_gpu_replay import _net, _store as game_store
    from test_gpu_value_targets import _valued
    B, K = 4, 3
    trajs = _valued()
    rp = game_store(N, trajs)
    search = dict(value_target="search", td_steps=2) if target == "search" else {}
    if ledger:                                             # (the trainer's own parameters: its call is then a no-op)
        rp.enable_position_priorities(2 if target == "search" else K, DISCOUNT, alpha=1.0, floor=1e-3)
    cfg = TrainConfig(unroll_steps=K, discount=DISCOUNT, device_sampling=True, sample_priorities=True,
                      importance_beta=0.5, fused_unroll=fused, fused_loss=fused, position_priorities=position,
                      priority_floor=1e-3 if position else 0.0, **search)
    tr = MuZeroTrainer(_net(N, C), cfg, mode="batched", sample_seed=11)
    out = dict(losses=[], items=[], pos=[], lengths=[len(t["actions"]) for t in trajs])
    for step in range(steps):
        if ledger:
            out["pos"].append(_np(rp.position_priorities()))
            if position:
                out["items"].append(rp.sample_positions_host(B, seed=11, step=step, beta=0.5)["items"])
        out["losses"].append(tr.train(rp, B))
    if ledger:
        out["pos"].append(_np(rp.position_priorities()))
    out["prio"] = _np(rp.device_priorities())
    out["params"] = [p.detach().clone() for p in tr.net.parameters()]
    out["skipped"] = rp.skipped_updates()
    return out


# latent_dim 32 trains on search-value targets (the 5x5 engine that network targets bootstrap from is built
# for C = 96 only); the third case is the network-target assembly at C = 96
@pytest.mark.parametrize("fused,C,target", [(True, 32, "search"), (False, 32, "search"), (True, 96, "network")])
def test_train_steps_with_position_priorities(fused, C, target):
    K = 3
    # (the torch path's conv backward: the deterministic algorithms, so that a repeat gives the same bits)
    flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a = _run(fused, C, target, True, True)
        b = _run(fused, C, target, True, True)
        plain = _run(fused, C, target, False, False)       # the game-level step, no ledger on the store
        held = _run(fused, C, target, False, True)         # ... and with one, switched off in the trainer
    finally:
        torch.backends.cudnn.deterministic = flag
    assert len(a["losses"]) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in a["losses"])
    assert a["skipped"] == 0
    # the stored weights changed on the sampled windows only
    lengths = a["lengths"]
    for step in range(3):
        was, now = a["pos"][step], a["pos"][step + 1]
        window = {(int(s), int(st) + k) for s, st, _ in a["items"][step] for k in range(K + 1)}      # (slot = game here)
        changed = 0
        for g, L in enumerate(lengths):
            for t in range(L):
                if (g, t) in window:
                    changed += now[g, t] != was[g, t]
                    assert now[g, t] >= 1e-3 and np.isfinite(now[g, t])
                else:
                    assert now[g, t] == was[g, t], (step, g, t)
        assert changed > 0
    np.testing.assert_array_equal(a["prio"], np.ones(len(lengths)))    # the per-game update did not run
    # a repeat from the same seed: the same bits
    assert a["losses"] == b["losses"]
    for x, y in zip(a["items"], b["items"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(_u64(a["pos"][-1]), _u64(b["pos"][-1]))
    for p, q in zip(a["params"], b["params"]):
        assert torch.equal(p, q)
    # position_priorities off: the parent's step, whether or not the store keeps position weights
    assert plain["losses"] == held["losses"] and plain["losses"] != a["losses"]
    np.testing.assert_array_equal(_u64(plain["prio"]), _u64(held["prio"]))
    assert (plain["prio"] != 1.0).any()
    for p, q in zip(plain["params"], held["params"]):
        assert torch.equal(p, q)
    np.testing.assert_array_equal(_u64(held["pos"][0]), _u64(held["pos"][-1]))     # and the position weights stay


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_a_store_without_the_ledger_refuses_every_new_call():
    import mzgo
    rp = mzgo.DeviceReplay(N, 4, 12, "cuda")
    for k, T in enumerate((3, 5)):
        rp.add(_game(T, k))
    s = rp.sample(2, seed=1, step=0)
    v = torch.zeros(2, 4, device="cuda")
    calls = (lambda: rp.sample_positions(2, seed=1, step=0),
             lambda: rp.sample_positions_batch(2, 3, DISCOUNT, seed=1, step=0),
             lambda: rp.sample_positions_batch_values(2, 3, 2, DISCOUNT, seed=1, step=0),
             lambda: rp.update_position_priorities(s, v, v),
             lambda: rp.position_priorities(),
             lambda: rp.set_position_priorities(np.ones((2, 12))),
             lambda: rp.sample_positions_host(2, seed=1, step=0))
    for call in calls:
        with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: .*mzgo_replay_enable_positions"):
            call()
    # enabling
    for kwargs, word in ((dict(td_steps=0), "td_steps"), (dict(alpha=0.0), "alpha"), (dict(floor=-1.0), "floor"),
                         (dict(discount=float("nan")), "discount")):
        a = dict(td_steps=3, discount=DISCOUNT)
        a.update(kwargs)
        with pytest.raises(mzgo.MzgoError, match=word):
            rp.enable_position_priorities(**a)
    with pytest.raises(ValueError, match="init"):
        rp.enable_position_priorities(3, DISCOUNT, init="loss")
    rp.enable_position_priorities(3, DISCOUNT, alpha=0.5)
    rp.enable_position_priorities(3, DISCOUNT, alpha=0.5)
    with pytest.raises(mzgo.MzgoError, match="already enabled with other parameters"):
        rp.enable_position_priorities(4, DISCOUNT, alpha=0.5)
    assert rp.sample_positions(2, seed=1, step=0)["items"].shape == (2, 3)
    with pytest.raises(mzgo.MzgoError, match="exceeds the 2 stored games"):
        rp.sample_positions(3, seed=1, step=0)
    for bad, word in ((-1.0, "finite values >= 0"), (float("nan"), "finite values >= 0"), (0.0, "no position")):
        w = np.ones((2, 12))
        w[1, :5] = bad
        with pytest.raises(mzgo.MzgoError, match=word):
            rp.set_position_priorities(w)
    w = np.ones((2, 12))
    w[1, 1:5] = 0.0                                                     # zeros on single positions are allowed
    rp.set_position_priorities(w)
    assert (_np(rp.sample_positions(2, seed=1, step=0)["items"])[:, 0] >= 0).all()
    long = mzgo.DeviceReplay(2, 1, 4097, "cuda")                        # the store itself has no such limit
    with pytest.raises(mzgo.MzgoError, match="max_moves 4097"):
        long.enable_position_priorities(3, DISCOUNT)
    long.close()
    big = mzgo.DeviceReplay(2, 64 ** 3 + 1, 1, "cuda")
    with pytest.raises(mzgo.MzgoError, match=r"64\^3"):
        big.enable_position_priorities(3, DISCOUNT)
    big.close()
