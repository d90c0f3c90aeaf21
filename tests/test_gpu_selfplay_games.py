"""Continuous self-play on the GPU: ``play_games_into(replay, n)`` -- n games on
G engine slots from one device queue (k_selfplay_games), finished games
ingested by the workgroup that played them (mzgo_replay_play_games).

The expected store is the path this replaces, on a second engine and store
with the same net, seed and game_base: ceil(n / G) epochs of ``reset(epoch)``
+ ``move(max_moves)`` + ``add_games``.  Queue game j is slot j % G of epoch
j // G, so game j of the one store must be game j of the other, byte for byte
through ``DeviceReplay.export`` (of the last epoch only its first n % G games
are compared when n % G != 0).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _net(N, C, seed=4):
    import mzgo
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A).cuda().eval()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, seed))
    return net


def _assert_same_game(got, want, N):
    """tests/test_gpu_replay.py's checks, plus the root values' bits and the key id."""
    T = len(want["actions"])
    assert len(got["observations"]) == len(want["observations"]) == T + 2
    for a, b in zip(got["observations"], want["observations"]):
        assert a.dtype == np.float64 and a.shape == (6, N, N)
        np.testing.assert_array_equal(a, np.asarray(b))
    assert got["actions"] == [int(a) for a in want["actions"]]
    assert len(got["rewards"]) == T + 1
    np.testing.assert_array_equal(np.array(got["rewards"]).view(np.uint64),
                                  np.array(want["rewards"], dtype=np.float64).view(np.uint64))
    assert len(got["policies"]) == T
    np.testing.assert_array_equal(np.array(got["policies"]).view(np.uint64),
                                  np.array(want["policies"], dtype=np.float64).view(np.uint64))
    assert len(got["root_values"]) == T
    np.testing.assert_array_equal(np.array(got["root_values"], dtype=np.float64).view(np.uint64),
                                  np.array(want["root_values"], dtype=np.float64).view(np.uint64))
    assert got["key_gid"] == want["key_gid"]


def _main_sp(N=6, C=128, G=4, S=16, seed=3, game_base=0, net_seed=5):
    """main.py's variant (MainSelfPlay); returns the SelfPlay under it."""
    from mzgo.trainer import MainSelfPlay
    return MainSelfPlay(_net(N, C, net_seed), G, S, seed=seed, game_base=game_base)


def _expected(sp, n, epoch0=0):
    """The parent path: whole epochs into a store of their own."""
    import mzgo
    epochs = -(-n // sp.G)
    rp = mzgo.DeviceReplay(sp.N, epochs * sp.G, sp.max_moves, "cuda")
    for e in range(epochs):
        sp.reset(epoch0 + e)
        sp.move(sp.max_moves)
        rp.add_games(sp.engine)
    return rp


def _assert_same_store(got, want, n, N, at=0):
    """games at .. at+n-1 of ``got`` are games 0 .. n-1 of ``want``"""
    assert len(got) >= at + n and len(want) >= n
    assert got.lengths[at:at + n] == want.lengths[:n]
    assert got.key_gids[at:at + n] == want.key_gids[:n]
    for j in range(n):
        _assert_same_game(got.export(at + j), want.export(j), N)


def _check(make, n, game_base=0):
    """play_games_into(n) on one engine against _expected on another; returns
    (SelfPlay, store, expected store)."""
    import mzgo
    from mzgo.replay import queue_key_gids
    a, b = make(), make()
    spa, spb = getattr(a, "sp", a), getattr(b, "sp", b)
    want = _expected(spb, n)
    rp = mzgo.DeviceReplay(spa.N, n, spa.max_moves, "cuda")
    c0 = spa.engine.counters()
    a.play_games_into(rp, n)
    assert len(rp) == n and spa.epoch == -(-n // spa.G)
    _assert_same_store(rp, want, n, spa.N)
    assert rp.key_gids == [int(x) for x in queue_key_gids(n, spa.G, game_base, 0)]
    # counters: a move's simulations, the moves, the games; one count per workgroup
    c1 = spa.engine.counters()
    moves = sum(rp.lengths)
    assert c1["moves"] - c0["moves"] == moves and c1["simulations"] - c0["simulations"] == moves * spa.S
    assert c1["games_finished"] - c0["games_finished"] == n
    assert c1["workgroups_started"] - c0["workgroups_started"] == min(n, spa.G)
    return spa, rp, want


# ---------------------------------------------------------------------------
# 1. main.py's variant: several games per workgroup, n % G != 0, n < G
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 10])
def test_main_variant_equals_whole_epochs(n):
    _check(_main_sp, n)


def test_fewer_games_than_slots_leaves_the_idle_slot_untouched():
    import mzgo
    msp, ref = _main_sp(), _main_sp()
    sp, eng = msp.sp, msp.sp.engine
    # slot 3 holds a finished game of its own (epoch 7) before the call
    sp.reset(7)
    sp.move(sp.max_moves)
    before, board = eng.record(3), eng.board_planes().cpu().numpy()[3]
    assert before["status"] == 1 and before["length"] >= 1
    sp.epoch = 0
    want = _expected(ref.sp, 3)
    rp = mzgo.DeviceReplay(sp.N, 4, sp.max_moves, "cuda")
    msp.play_games_into(rp, 3)
    assert len(rp) == 3 and sp.epoch == 1
    _assert_same_store(rp, want, 3, sp.N)
    after = eng.record(3)
    assert after["status"] == before["status"] and after["length"] == before["length"]
    for k in ("stones", "invd", "flags", "action", "reward"):
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    for k in ("value", "policy"):
        np.testing.assert_array_equal(after[k].view(np.uint64), before[k].view(np.uint64), err_msg=k)
    assert after["final_reward"] == before["final_reward"]
    np.testing.assert_array_equal(eng.board_planes().cpu().numpy()[3], board)


# ---------------------------------------------------------------------------
# 2. compat "fixed", self_play.py's variant (the move reads the search)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,temperature", [(9, 1.0), (5, 0.5)])
def test_fixed_compat_equals_whole_epochs(N, temperature):
    import mzgo
    make = lambda: mzgo.SelfPlay(_net(N, 96), 3, 24, seed=11, compat="fixed", max_moves=12,
                                 temperature=temperature, game_base=5)
    _check(make, 7, game_base=5)


# ---------------------------------------------------------------------------
# 3. compat "reference": both ways a game ends, both reward rules of the ingest
# ---------------------------------------------------------------------------
def test_reference_compat_games_end_both_ways():
    import mzgo
    # seed 2: of games 0..11 (slot j % 4 of epoch j // 4), games 4 and 8 reach the
    # move cap and the others end by double pass -- the board sequences read no
    # network (tests/test_selfplay_games.py plays them on the CPU)
    make = lambda: mzgo.SelfPlay(_net(5, 96), 4, 8, seed=2, compat="reference", max_moves=60)
    _, rp, want = _check(make, 12)
    done = [bool(want.export(j)["observations"][-1][5].max() > 0) for j in range(12)]
    capped = [L == 60 and not d for L, d in zip(want.lengths, done)]
    assert any(done) and any(capped)
    for j in range(12):
        rewards = rp.export(j)["rewards"]
        if capped[j]:
            assert rewards[-2] == -0.5 and rewards[-1] == 0.0     # the move-cap rule; no winner
        if done[j]:
            assert rewards[-1] == rewards[-2]                      # the winner, last (and the last move's reward)


# ---------------------------------------------------------------------------
# 4. 19x19: trees in HBM, lazy rows, no helper workgroups
# ---------------------------------------------------------------------------
def test_19x19_equals_whole_epochs():
    import mzgo
    make = lambda: mzgo.SelfPlay(_net(19, 96), 2, 24, seed=6, compat="fixed", max_moves=6)
    _check(make, 5)


# ---------------------------------------------------------------------------
# 5. a wrapping ring
# ---------------------------------------------------------------------------
def test_games_wrap_the_ring_in_index_order():
    import mzgo
    from mzgo._lib import lib
    from oracle.make_golden import synthetic_trajectories
    N = 6
    trajs = synthetic_trajectories(N, 5, seed=9)
    msp, ref = _main_sp(), _main_sp()
    rp = mzgo.DeviceReplay(N, 8, msp.max_moves, "cuda")
    for k, t in enumerate(trajs):
        rp.add(t, key_gid=100 + k)
    want = _expected(ref.sp, 6)
    msp.play_games_into(rp, 6)
    assert len(rp) == 8 and rp.key_gids[:2] == [103, 104]
    for i, t in enumerate(trajs[3:]):                     # the 3 oldest were evicted
        got = rp.export(i)
        assert got["actions"] == [int(a) for a in t["actions"]] and got["key_gid"] == 103 + i
        for a, b in zip(got["observations"], t["observations"]):
            np.testing.assert_array_equal(a, np.asarray(b))
    _assert_same_store(rp, want, 6, N, at=2)
    size, head = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mzgo_replay_info(rp.handle, ctypes.byref(size), ctypes.byref(head), None, None) == 0
    assert (size.value, head.value) == (8, 3)


# ---------------------------------------------------------------------------
# 6. the stored key ids are the records' own search keys
# ---------------------------------------------------------------------------
def test_reanalysis_under_the_same_weights_keeps_every_root_value():
    import mzgo
    from mzgo.reanalyse import Reanalyser
    msp = _main_sp()
    rp = mzgo.DeviceReplay(msp.N, 12, msp.max_moves, "cuda")
    msp.play_games_into(rp, 12)
    before = [rp.export(j) for j in range(12)]
    rp.reanalyse(Reanalyser(msp.sp.net, 16, slots=4, seed=3))
    torch.cuda.synchronize()
    assert sum(len(b["actions"]) for b in before) >= 12
    for j, b in enumerate(before):
        got = rp.export(j)
        np.testing.assert_array_equal(np.array(got["root_values"], dtype=np.float64).view(np.uint64),
                                      np.array(b["root_values"], dtype=np.float64).view(np.uint64))
        assert got["actions"] == b["actions"] and got["key_gid"] == b["key_gid"]


# ---------------------------------------------------------------------------
# 7. the epoch sequence goes on
# ---------------------------------------------------------------------------
def test_play_into_continues_the_epoch_sequence():
    import mzgo
    from mzgo.reanalyse import record_ids
    msp, ref = _main_sp(), _main_sp()
    rp = mzgo.DeviceReplay(msp.N, 14, msp.max_moves, "cuda")
    msp.play_games_into(rp, 10)
    assert msp.sp.epoch == 3
    msp.play_into(rp)
    assert len(rp) == 14 and msp.sp.epoch == 4
    assert rp.key_gids[10] == rp.export(10)["key_gid"] == record_ids(0, 0, 3, [0])[0, 0]
    # ... and that game is the epoch path's own
    want = mzgo.DeviceReplay(msp.N, 4, msp.max_moves, "cuda")
    ref.sp.epoch = 3
    ref.play_into(want)
    _assert_same_store(rp, want, 4, msp.N, at=10)


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals():
    import mzgo
    from mzgo import Engine, EngineConfig
    from mzgo._lib import MZGO_EINVAL, lib, stream_of
    from oracle.make_golden import synthetic_trajectories
    N, M = 5, 15
    trajs = synthetic_trajectories(N, 2, seed=9)
    trajs = [t for t in trajs if len(t["actions"]) <= M]
    assert trajs
    rp = mzgo.DeviceReplay(N, 3, M, "cuda")
    for k, t in enumerate(trajs):
        rp.add(t, key_gid=50 + k)
    held = len(rp)
    snapshot = [rp.export(i) for i in range(held)]
    net = _net(N, 96)
    sp = mzgo.SelfPlay(net, 2, 4, seed=1, compat="fixed", max_moves=M)
    eng = sp.engine
    s = stream_of(rp.device)

    def refused(handle, e, n, word):
        assert lib.mzgo_replay_play_games(handle, e.handle if e is not None else None, n, 0, s) == MZGO_EINVAL
        msg = lib.mzgo_last_error().decode()
        assert "mzgo_replay_play_games" in msg and word in msg, msg
        size = ctypes.c_int32(-1)
        assert lib.mzgo_replay_info(rp.handle, ctypes.byref(size), None, None, None) == 0 and size.value == held
        assert len(rp) == held
        for i, want in enumerate(snapshot):
            got = rp.export(i)
            assert got["actions"] == want["actions"] and got["key_gid"] == want["key_gid"]
            np.testing.assert_array_equal(np.array(got["policies"]), np.array(want["policies"]))
            for a, b in zip(got["observations"], want["observations"]):
                np.testing.assert_array_equal(a, b)

    refused(rp.handle, eng, 0, "n_games must be >= 1")
    refused(rp.handle, eng, 4, "exceeds the capacity")
    refused(None, eng, 1, "null replay")
    refused(rp.handle, None, 1, "null engine")
    refused(rp.handle, Engine(EngineConfig(board_size=N, latent_dim=0, num_games=2)), 1, "board-only")
    refused(rp.handle, Engine(EngineConfig(board_size=N, latent_dim=64, num_games=2, num_simulations=4, tower=1,
                                           res_blocks=1)), 1, "tower")
    refused(rp.handle, net.engine(2, 4, max_moves=M + 1), 1, "max_moves mismatch")
    refused(rp.handle, _net(6, 96).engine(2, 4, max_moves=M), 1, "board size mismatch")
    eng.inject_noise(torch.full((2, M, N * N + 1), 1.0 / (N * N + 1), dtype=torch.float64))
    refused(rp.handle, eng, 1, "noise hook")
    eng.inject_noise(None)
    buf = torch.zeros(2, M, N * N + 1, dtype=torch.float64, device="cuda")
    eng.record_noise(buf)
    refused(rp.handle, eng, 1, "noise hook")
    eng.record_noise(None)
    with pytest.raises(mzgo.MzgoError, match="exceeds the capacity"):
        sp.play_games_into(rp, 4)
    assert sp.epoch == 0 and len(rp) == held
    # the slots after a call: games of several epochs
    sp.play_games_into(rp, 3)
    assert len(rp) == 3 and sp.epoch == 2
    with pytest.raises(RuntimeError, match="several epochs"):
        sp.reanalyse()
    with pytest.raises(RuntimeError, match="several epochs"):
        sp.histories()
    sp.reset()
    sp.move(M)
    out = sp.reanalyse()
    assert len(out) == 2 and len(sp.histories()) == 2
    for g, (visits, value, policy) in enumerate(out):
        rec = eng.record(g)
        np.testing.assert_array_equal(value.view(np.uint64), rec["value"].view(np.uint64))
