"""The device replay store on the GPU (mzgo.DeviceReplay, csrc/mzgo_replay.hip).

Everything is compared bit for bit with the host path it replaces --
``PrioritizedReplayBuffer`` + ``MuZeroTrainer.batch_targets`` + ``Reanalyser.run``
over main.py-format trajectories -- except the loss of a whole step, which is
two orders of the same float32 sums (rel 1e-4, as
test_batched_bootstrap_on_hip_equals_torch allows).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 10                                           # TrainConfig.unroll_steps


def _net(N, C, seed=4):
    import mzgo
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, seed))
    return net


_TRAJS = {}


def _trajs(N, B=6):
    """synthetic_trajectories (T <= 15), made once per shape and never changed.
    Seed 9 gives 5x5 games of 9, 9, 8, 9, 15, 7 moves and 6x6 games of 9, 5, 14,
    3, 13, 12; the two 9x9 games (seed 10) have 13 moves and 2: with K = 10
    every shape has samples with and without bootstrap positions."""
    from oracle.make_golden import synthetic_trajectories
    if (N, B) not in _TRAJS:
        _TRAJS[N, B] = synthetic_trajectories(N, B, seed=10 if N == 9 else 9)
    return _TRAJS[N, B]


def _store(N, trajs, capacity=None, max_moves=None, gid0=100):
    import mzgo
    rp = mzgo.DeviceReplay(N, capacity or len(trajs), max_moves or int(1.5 * N * N), "cuda")
    for k, t in enumerate(trajs):
        rp.add(t, key_gid=gid0 + k)
    return rp


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint8)


def _assert_same_bits(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=name)


def _assert_same_game(got, want, N):
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


def _starts(trajs):
    """Every game from its first move, its last and a middle one."""
    idx, st = [], []
    for g, t in enumerate(trajs):
        T = len(t["actions"])
        for s in (0, T - 1, T // 2):
            idx.append(g)
            st.append(s)
    return idx, st


# ---------------------------------------------------------------------------
# 1. round trip, eviction, the ring's wrap
# ---------------------------------------------------------------------------
def test_round_trip_through_a_wrapping_ring():
    from mzgo.trainer import PrioritizedReplayBuffer
    N = 5
    trajs = _trajs(N)
    rp = _store(N, trajs, capacity=4)
    assert len(rp) == 4 and rp.lengths == [len(t["actions"]) for t in trajs[2:]]
    assert rp.key_gids == [102, 103, 104, 105] and rp.priorities == [1.0] * 4
    for i, want in enumerate(trajs[2:]):         # games 0 and 1 were evicted
        got = rp.export(i)
        _assert_same_game(got, want, N)
        assert got["root_values"] == [0.0] * len(want["actions"]) and got["key_gid"] == 102 + i
    _assert_same_game(rp.export(-1), trajs[-1], N)
    with_values = dict(trajs[0], root_values=[0.25 * t for t in range(len(trajs[0]["actions"]))])
    rp.add(with_values, key_gid=-7)
    assert rp.export(3)["root_values"] == with_values["root_values"] and rp.export(3)["key_gid"] == -7
    _assert_same_game(rp.export(0), trajs[3], N)
    # the ledger draws main.py's indices after eviction and a priority update
    buf = PrioritizedReplayBuffer(4)
    for t in trajs + [with_values]:
        buf.add(t)
    rp.update_priorities([1, 2], [3.0, 0.5])
    buf.update_priorities([1, 2], [3.0, 0.5])
    np.random.seed(3)
    want = buf.sample(3)[1]
    np.random.seed(3)
    np.testing.assert_array_equal(rp.sample_indices(3), want)
    with pytest.raises(ValueError):
        rp.add(dict(trajs[0], actions=list(range(38)), policies=[trajs[0]["policies"][0]] * 38))


# ---------------------------------------------------------------------------
# 2. batch assembly equals the host target builder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,B", [(5, 96, 6), (6, 128, 6), (9, 96, 2)])
def test_batch_equals_host_targets(N, C, B):
    from mzgo.trainer import MuZeroTrainer
    trajs = _trajs(N, B)
    net = _net(N, C)
    tr = MuZeroTrainer(net, mode="batched")
    assert tr.config.unroll_steps == K
    rp = _store(N, trajs)
    idx, starts = _starts(trajs)
    want = tr.host_targets([trajs[g] for g in idx], starts)
    got = tr.device_targets(rp, idx, starts)
    for name, g, w in zip(("obs0", "acts", "t_val", "t_rew", "t_pol"), got, want):
        _assert_same_bits(g, w, name)
    # both branches of every "past the end" rule were crossed
    bt = rp.batch(idx, starts, K, tr.config.discount)
    hb = bt["has_boot"].cpu().numpy()
    assert hb.any() and not hb.all()
    A = N * N + 1
    lens = np.array([len(trajs[g]["actions"]) for g in idx])
    past = (np.array(starts)[:, None] + np.arange(K)[None, :]) >= lens[:, None]
    assert past.any() and not past.all()
    assert (bt["acts"].cpu().numpy()[past] == A - 1).all()
    assert (bt["boot_obs"].cpu().numpy()[hb == 0] == 0).all()


# ---------------------------------------------------------------------------
# 3. the eight symmetries
# ---------------------------------------------------------------------------
def _sym(x, s):
    y = np.rot90(x, s & 3, axes=(-2, -1))
    return np.ascontiguousarray(np.flip(y, axis=-1) if s & 4 else y)


def _transformed(traj, s, N):
    C = N * N

    def pol(p):
        p = np.asarray(p)
        return np.concatenate([_sym(p[:C].reshape(N, N), s).reshape(-1), p[C:]])

    def act(a):
        if a >= C:
            return a
        hot = np.zeros(C)
        hot[a] = 1.0
        return int(np.argmax(_sym(hot.reshape(N, N), s)))

    return dict(observations=[_sym(np.asarray(o), s) for o in traj["observations"]],
                actions=[act(a) for a in traj["actions"]], rewards=list(traj["rewards"]),
                policies=[pol(p) for p in traj["policies"]])


def test_symmetries_equal_the_transformed_trajectory():
    from mzgo.trainer import MuZeroTrainer
    N, C = 5, 96
    trajs = _trajs(N)
    g = int(np.argmax([len(t["actions"]) for t in trajs]))        # the longest game: bootstrap rows exist
    traj, T = trajs[g], len(trajs[g]["actions"])
    assert T > K
    tr = MuZeroTrainer(_net(N, C), mode="batched")
    rp = _store(N, trajs)
    starts = [0, T - 1, T // 2]
    for s in range(8):
        moved = _transformed(traj, s, N)
        want = tr.host_targets([moved] * 3, starts)
        got = tr.device_targets(rp, [g] * 3, starts, [s] * 3)
        for name, a, b in zip(("obs0", "acts", "t_val", "t_rew", "t_pol"), got, want):
            if name != "t_val" or s == 0:        # the network is not symmetric: bootstrap values differ
                _assert_same_bits(a, b, name)
        bt = rp.batch([g] * 3, starts, K, tr.config.discount, [s] * 3)
        val, factor, hb = (bt[k].cpu().numpy() for k in ("val", "factor", "has_boot"))
        boot_obs = bt["boot_obs"].cpu().numpy()
        for b, st in enumerate(starts):
            for k in range(K + 1):
                v, f, boot = tr._discounted(moved, st + k)
                assert val[b, k] == v and factor[b, k] == f and bool(hb[b, k]) == (boot is not None)
                want_obs = moved["observations"][boot] if boot is not None else np.zeros((6, N, N))
                np.testing.assert_array_equal(boot_obs[b, k], want_obs.astype(np.float32))
    # a batch may mix symmetries
    mixed = rp.batch([g] * 8, [1] * 8, K, tr.config.discount, list(range(8)))
    for s in range(8):
        np.testing.assert_array_equal(mixed["obs0"][s].cpu().numpy(),
                                      _sym(np.asarray(traj["observations"][1]), s).astype(np.float32))


# ---------------------------------------------------------------------------
# 4. ingest from an engine, device to device
# ---------------------------------------------------------------------------
def test_engine_ingest_equals_trajectory_from_record():
    import mzgo
    from mzgo.reanalyse import record_ids
    from mzgo.trainer import MainSelfPlay, trajectory_from_record
    N, C, G, S = 6, 128, 8, 16
    net = _net(N, C, 5).eval()
    msp = MainSelfPlay(net, G, S, seed=3)
    rp = mzgo.DeviceReplay(N, 2 * G, msp.max_moves, "cuda")
    eng = msp.sp.engine
    msp.sp.reset()
    with pytest.raises(RuntimeError):            # every game still playing
        rp.add_games(eng)
    assert len(rp) == 0
    msp.play_into(rp)
    assert len(rp) == G and msp.sp.epoch == 1
    finals = eng.board_planes().cpu().numpy()
    for g in range(G):
        rec = eng.record(g)
        want = trajectory_from_record(rec, finals[g], N, msp.max_moves)
        got = rp.export(g)
        _assert_same_game(got, want, N)
        L = rec["length"]
        assert rp.lengths[g] == L >= 1
        np.testing.assert_array_equal(np.array(got["root_values"]), rec["value"][:L])
        assert got["key_gid"] == rp.key_gids[g] == record_ids(0, g, 0, [0])[0, 0]
        done = finals[g][5].max() > 0
        assert got["rewards"][-1] == (float(rec["final_reward"]) if done else 0.0)
        if not done:
            assert L == msp.max_moves and got["rewards"][-2] == rec["reward"][L - 1] - 0.5
    # a second epoch lands behind the first, keyed by its own epoch
    msp.play_into(rp)
    assert len(rp) == 2 * G and rp.key_gids[G] == record_ids(0, 0, 1, [0])[0, 0]
    _assert_same_game(rp.export(G + 1), trajectory_from_record(eng.record(1), eng.board_planes().cpu().numpy()[1], N,
                                                               msp.max_moves), N)


# ---------------------------------------------------------------------------
# 5. reanalysis in place
# ---------------------------------------------------------------------------
def test_reanalysis_in_place_equals_the_host_reanalyser():
    from mzgo.reanalyse import Reanalyser, record_ids
    N, C, S = 5, 96, 16
    trajs = _trajs(N)
    net = _net(N, C, 0).eval()
    ra = Reanalyser(net, S, slots=4, seed=13)
    rp = _store(N, trajs, gid0=100)
    rp.reanalyse(ra)
    ids = [record_ids(0, 100 + k, 0, np.arange(len(t["actions"]))) for k, t in enumerate(trajs)]
    want = ra.run(trajs, ids=ids)
    changed = 0
    for k, w in enumerate(want):
        got = rp.export(k)
        _assert_same_game(got, w, N)             # observations, actions, rewards untouched; policies fresh
        np.testing.assert_array_equal(np.array(got["root_values"]).view(np.uint64),
                                      np.array(w["root_values"], dtype=np.float64).view(np.uint64))
        changed += int(not np.array_equal(np.array(got["policies"]), np.array(trajs[k]["policies"])))
    assert changed == len(trajs)
    # a subset: only the named games change
    rp2 = _store(N, trajs, gid0=100)
    rp2.reanalyse(ra, games=[4, 1])
    for k in range(len(trajs)):
        _assert_same_game(rp2.export(k), want[k] if k in (1, 4) else trajs[k], N)


# ---------------------------------------------------------------------------
# 6. a whole step
# ---------------------------------------------------------------------------
def test_train_step_on_a_device_replay_equals_the_host_buffer():
    from mzgo.trainer import MuZeroTrainer, PrioritizedReplayBuffer, TrainConfig
    N, C, B = 5, 96, 4
    trajs = _trajs(N)
    rp = _store(N, trajs)
    buf = PrioritizedReplayBuffer(len(trajs))
    for t in trajs:
        buf.add(t)
    nets = [_net(N, C), _net(N, C)]
    start = lambda T: T // 3
    tr_h = MuZeroTrainer(nets[0], mode="batched", start_index=start)
    tr_d = MuZeroTrainer(nets[1], mode="batched", start_index=start)
    # the targets of the step both are about to take
    np.random.seed(0)
    idx = rp.sample_indices(B)
    starts = [start(rp.lengths[i]) for i in idx]
    want = tr_h.host_targets([trajs[i] for i in idx], starts)
    got = tr_d.device_targets(rp, idx, starts)
    for name, a, b in zip(("obs0", "acts", "t_val", "t_rew", "t_pol"), got, want):
        _assert_same_bits(a, b, name)
    before = {k: v.clone() for k, v in nets[1].state_dict().items()}
    np.random.seed(0)
    loss_h = tr_h.train(buf, B)
    np.random.seed(0)
    loss_d = tr_d.train(rp, B)
    assert np.isfinite(loss_d) and loss_d == pytest.approx(loss_h, rel=1e-4)
    for k in ("value_loss", "policy_loss", "reward_loss"):
        assert tr_d.last[k] == pytest.approx(tr_h.last[k], rel=1e-4, abs=1e-7)
    assert rp.priorities == pytest.approx(buf.priorities, rel=1e-4)
    assert sorted(np.flatnonzero(np.array(rp.priorities) != 1.0)) == sorted(idx)
    assert any(not torch.equal(before[k], v) for k, v in nets[1].state_dict().items())
    assert tr_d.scheduler.last_epoch == 1
    # too few games: no step, as the host buffers answer; reference mode says what it needs
    assert tr_d.train(rp, len(trajs) + 1) is None
    with pytest.raises(ValueError, match="batched"):
        MuZeroTrainer(nets[0], mode="reference").train(rp, B)
    # the symmetries flag: a step on randomly transformed samples
    tr_s = MuZeroTrainer(nets[1], TrainConfig(symmetries=True), mode="batched", start_index=start)
    assert np.isfinite(tr_s.train(rp, B))


# ---------------------------------------------------------------------------
# 7. refusals, through ctypes
# ---------------------------------------------------------------------------
def test_refusals():
    import mzgo
    from mzgo import Engine, EngineConfig
    from mzgo._lib import MZGO_EINVAL, MZGO_OK, lib, ptr, stream_of
    N = 5
    A = N * N + 1
    trajs = _trajs(N)[:2]
    rp = _store(N, trajs, capacity=3)
    dev = rp.device
    T0 = len(trajs[0]["actions"])
    out = dict(obs0=torch.zeros(2, 6, N, N, device=dev), boot_obs=torch.zeros(2, K + 1, 6, N, N, device=dev),
               acts=torch.zeros(2, K, dtype=torch.int64, device=dev), t_rew=torch.zeros(2, K, device=dev),
               t_pol=torch.zeros(2, K + 1, A, device=dev), val=torch.zeros(2, K + 1, dtype=torch.float64, device=dev),
               factor=torch.zeros(2, K + 1, dtype=torch.float64, device=dev),
               has_boot=torch.zeros(2, K + 1, dtype=torch.uint8, device=dev))

    items = torch.zeros(2, 3, dtype=torch.int32, device=dev)

    # the samples' checks are mzgo_replay_items', the outputs' mzgo_replay_batch_items'
    def upload(handle=rp.handle, idx=(0, 1), starts=(0, 1), syms=None, B=2, it=items):
        i32 = lambda x: None if x is None else np.array(x, np.int32)
        a, b, c = i32(idx), i32(starts), i32(syms)
        rc = lib.mzgo_replay_items(handle, ptr(a), ptr(b), ptr(c), B, ptr(it), stream_of(dev))
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    def call(handle=rp.handle, it=items, B=2, unroll=K, drop=None):
        o = {k: (None if k == drop else ptr(v)) for k, v in out.items()}
        rc = lib.mzgo_replay_batch_items(handle, ptr(it), B, unroll, 0.99, o["obs0"], o["boot_obs"], o["acts"],
                                         o["t_rew"], o["t_pol"], o["val"], o["factor"], o["has_boot"], stream_of(dev))
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    assert upload()[0] == MZGO_OK and call()[0] == MZGO_OK
    assert items.cpu().tolist() == [[0, 0, 0], [1, 1, 0]]
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(B=0), "B must be >= 1"),
                         (dict(idx=None), "null indices"), (dict(starts=None), "null starts"),
                         (dict(it=None), "null items"),
                         (dict(idx=(0, 2)), "game 2 is not in the store"), (dict(idx=(-1, 0)), "game -1"),
                         (dict(starts=(T0, 0)), f"start {T0} outside"), (dict(starts=(0, -1)), "start -1 outside"),
                         (dict(syms=(0, 8)), "symmetry 8"), (dict(syms=(-1, 0)), "symmetry -1")):
        rc, msg = upload(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_items" in msg and word in msg, (kwargs, rc, msg)
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(B=0), "B must be >= 1"),
                         (dict(it=None), "null items"),
                         (dict(drop="t_pol"), "null t_pol"), (dict(drop="has_boot"), "null has_boot"),
                         (dict(unroll=0), "unroll_steps 0"), (dict(unroll=64), "unroll_steps 64")):
        rc, msg = call(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_batch_items" in msg and word in msg, (kwargs, rc, msg)
    with pytest.raises((mzgo.MzgoError, IndexError)):
        rp.batch([0, 5], [0, 0], K, 0.99)
    # ingest: engines the store cannot take
    net = _net(N, 96)
    s = stream_of(dev)
    for eng, word in ((Engine(EngineConfig(board_size=N, latent_dim=0, num_games=2)), "board-only"),
                      (Engine(EngineConfig(board_size=N, latent_dim=64, num_games=2, num_simulations=4, tower=1,
                                           res_blocks=1)), "tower"),
                      (net.engine(2, 4, max_moves=int(1.5 * N * N) - 1), "max_moves mismatch"),
                      (_net(6, 96).engine(2, 4, max_moves=int(1.5 * N * N)), "board size mismatch")):
        assert lib.mzgo_replay_add_games(rp.handle, eng.handle, s) == MZGO_EINVAL
        assert word in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_add_games(None, net.engine(2, 4).handle, s) == MZGO_EINVAL
    assert lib.mzgo_replay_add_games(rp.handle, None, s) == MZGO_EINVAL
    assert "null engine" in lib.mzgo_last_error().decode()
    assert len(rp) == 2                          # nothing was taken
    # the other entry points
    assert lib.mzgo_replay_export(rp.handle, 2, None, None, None, None, None, None, None, None, None, s) == MZGO_EINVAL
    assert "game 2 out of range" in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_export(None, 0, None, None, None, None, None, None, None, None, None, s) == MZGO_EINVAL
    assert lib.mzgo_replay_add(rp.handle, 1000, None, None, None, None, None, None, None, 0, s) == MZGO_EINVAL
    assert "length 1000 out of range" in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_add(rp.handle, 1, None, None, None, None, None, None, None, 0, s) == MZGO_EINVAL
    assert "null stones" in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_finish_values(None, None, None, None, 4, None, s) == MZGO_EINVAL
    assert lib.mzgo_replay_finish_values(ptr(out["val"]), ptr(out["factor"]), ptr(out["has_boot"]), ptr(out["t_rew"]),
                                         0, ptr(out["t_rew"]), s) == MZGO_EINVAL
    games = np.array([0, 7], np.int32)
    six = _net(6, 96).engine(2, 4, compat="fixed")
    assert lib.mzgo_replay_reanalyse(rp.handle, six.handle, None, 0, s) == MZGO_EINVAL
    assert "board size mismatch" in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_reanalyse(rp.handle, net.engine(2, 4, compat="fixed").handle, ptr(games), 2, s) == MZGO_EINVAL
    assert "game 7 is not in the store" in lib.mzgo_last_error().decode()
    assert lib.mzgo_replay_reanalyse(None, six.handle, None, 0, s) == MZGO_EINVAL
    size = ctypes.c_int32(-1)
    assert lib.mzgo_replay_info(rp.handle, ctypes.byref(size), None, None, None) == MZGO_OK and size.value == 2
    assert lib.mzgo_replay_info(None, ctypes.byref(size), None, None, None) == MZGO_EINVAL
