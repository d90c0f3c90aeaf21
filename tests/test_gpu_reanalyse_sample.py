"""Reanalysis of a sampled batch's windows on the GPU (mzgo.DeviceReplay
``reanalyse_sample`` / ``batch_from``; csrc/mzgo_replay.hip:
k_replay_window_items; csrc/mzgo_kernels.hpp: k_reanalyse_queue<N, C, true>)
and ``TrainConfig.reanalyse_sample``.

The in-place queue searches a position under the key whole-game reanalysis
(``DeviceReplay.reanalyse``) gives it, so inside a batch's windows the policy
rows and root values of the two must agree bit for bit, and outside them the
store must hold what it held.  test_gpu_replay's shapes: 5x5, C = 96, 16
simulations, four tree slots, the six synthetic games of 9, 9, 8, 9, 15 and 7
moves.  A whole trainer step is held to test_gpu_replay's bar for one (loss
rel 1e-4).
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_replay import _assert_same_bits, _net, _store, _trajs
from test_window_items import restated_items

pytestmark = pytest.mark.gpu

N, C, S = 5, 96, 16
GID0 = 100


def _np(t):
    return t.cpu().numpy()


def _reanalyser(net):
    from mzgo.reanalyse import Reanalyser
    return Reanalyser(net, S, slots=4, seed=13)


def _rows(rp):
    """The store's games as exported: per game (policies [L, A], root values [L]) as uint64 bits."""
    out = []
    for k in range(len(rp)):
        g = rp.export(k)
        L = len(g["actions"])
        out.append((np.array(g["policies"], dtype=np.float64).reshape(L, -1).view(np.uint64),
                    np.array(g["root_values"], dtype=np.float64).view(np.uint64)))
    return out


@functools.lru_cache(maxsize=None)
def _whole_games():
    """(the net, its reanalyser, the rows before, the rows after every game was
    reanalysed as a whole game): made once, never changed."""
    trajs = _trajs(N)
    net = _net(N, C, 0).eval()
    ra = _reanalyser(net)
    rp = _store(N, trajs, gid0=GID0)
    before = _rows(rp)
    rp.reanalyse(ra)
    after = _rows(rp)
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(before, after))
    return net, ra, before, after


def _check_windows(rp, ra, items, K, before, after):
    """reanalyse_sample on ``rp`` for the device ``items``; then every row of
    the windows holds whole-game reanalysis' bits and every other row, and
    every other field, what it held."""
    trajs = _trajs(N)
    prio, gen = _np(rp.device_priorities()), _np(rp.device_generations())
    n = rp.reanalyse_sample(ra, items, K)
    assert n.is_cuda and n.dtype == torch.int32 and n.shape == (1,)
    host_items = _np(items["items"] if isinstance(items, dict) else items)
    want = rp.window_items_host(host_items, K)
    np.testing.assert_array_equal(want, restated_items(rp.lengths, host_items, K))   # (slot = logical index here)
    assert n.item() == len(want) > 0
    inside = {(int(s), int(t)) for s, t in want}
    got = _rows(rp)
    hit = 0
    for k, t in enumerate(trajs):
        g = rp.export(k)
        L = len(t["actions"])
        assert len(g["actions"]) == L == rp.lengths[k] and g["key_gid"] == GID0 + k == rp.key_gids[k]
        assert g["actions"] == [int(a) for a in t["actions"]]
        np.testing.assert_array_equal(np.array(g["rewards"]).view(np.uint64),
                                      np.array(t["rewards"], dtype=np.float64).view(np.uint64))
        for a, b in zip(g["observations"], t["observations"]):
            np.testing.assert_array_equal(a, np.asarray(b))
        for row in range(L):
            src = after if (k, row) in inside else before
            hit += (k, row) in inside
            np.testing.assert_array_equal(got[k][0][row], src[k][0][row], err_msg=f"policy of game {k} move {row}")
            assert got[k][1][row] == src[k][1][row], f"root value of game {k} move {row}"
    assert hit == len(inside)
    np.testing.assert_array_equal(_np(rp.device_priorities()), prio)
    np.testing.assert_array_equal(_np(rp.device_generations()), gen)
    return inside


# ---------------------------------------------------------------------------
# 1. the windows equal whole-game reanalysis; the rest is untouched
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 10])
def test_sampled_windows_equal_whole_game_reanalysis(K):
    net, ra, before, after = _whole_games()
    trajs = _trajs(N)
    rp = _store(N, trajs, gid0=GID0)
    rp.set_device_priorities(np.linspace(0.5, 3.0, len(trajs)))
    s = rp.sample(4, seed=8, step=K, symmetries=True)
    inside = _check_windows(rp, ra, s, K, before, after)
    total = sum(len(t["actions"]) for t in trajs)
    assert 0 < len(inside) < total                               # some rows searched, some left alone


@pytest.mark.parametrize("K", [3, 10])
def test_hand_made_windows_equal_whole_game_reanalysis(K):
    net, ra, before, after = _whole_games()
    trajs = _trajs(N)
    lens = [len(t["actions"]) for t in trajs]
    # every game but the last from its first move, its last and a middle one
    # (overlapping windows: a row listed twice is searched twice, to the same
    # bits); then triples that contribute nothing
    triples = [(k, st, (k + st) % 8) for k, L in enumerate(lens[:-1]) for st in (0, L - 1, L // 2)]
    triples += [(-1, 0, 0), (len(trajs), 0, 0), (0, lens[0], 0), (1, -1, 0)]
    items = torch.tensor(triples, dtype=torch.int32, device="cuda")
    rp = _store(N, trajs, gid0=GID0)
    inside = _check_windows(rp, ra, items, K, before, after)
    assert all((k, L - 1) in inside and (k, 0) in inside for k, L in enumerate(lens[:-1]))
    assert not any(k == len(trajs) - 1 for k, _ in inside)       # the last game keeps every row
    if K == 3:
        assert (4, 5) not in inside and (4, 11) not in inside         # 15 moves: rows 0..3, 7..10 and 14


# ---------------------------------------------------------------------------
# 2. sample + batch_from = sample_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("symmetries", [False, True])
def test_batch_from_equals_sample_batch(symmetries):
    trajs = _trajs(N)
    B, K = len(trajs), 10
    rp = _store(N, trajs)
    rp.set_device_priorities(np.linspace(0.5, 3.0, B))
    for step in range(2):
        want = rp.sample_batch(B, K, 0.99, seed=8, step=step, symmetries=symmetries)
        s = rp.sample(B, seed=8, step=step, symmetries=symmetries)
        got = rp.batch_from(s, K, 0.99)
        assert set(got) == {"obs0", "boot_obs", "acts", "t_rew", "t_pol", "val", "factor", "has_boot"}
        for name in ("items", "index", "gen", "weight"):
            _assert_same_bits(s[name], want[name], name)
        for name, g in got.items():
            _assert_same_bits(g, want[name], name)
        for name, g in rp.batch_from(s["items"], K, 0.99).items():       # the items tensor alone
            _assert_same_bits(g, want[name], name)
    assert not symmetries or _np(s["items"])[:, 2].max() > 0


# ---------------------------------------------------------------------------
# 3. a whole step
# ---------------------------------------------------------------------------
def test_train_step_with_reanalyse_sample():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    trajs = _trajs(N)
    B, K, seed = 4, 3, 5                                         # (K = 3: late starts clip at L - 1, early ones do not)
    prio = np.linspace(0.5, 3.0, len(trajs))
    stores = [_store(N, trajs, gid0=GID0) for _ in range(3)]
    for rp in stores:
        rp.set_device_priorities(prio)
    rp_on, rp_off, rp_direct = stores
    nets = [_net(N, C), _net(N, C), _net(N, C)]
    tr_on = MuZeroTrainer(nets[0], TrainConfig(unroll_steps=K, device_sampling=True, reanalyse_sample=True,
                                               reanalyse_every=2), mode="batched", sample_seed=seed,
                          reanalyser=_reanalyser(nets[0]))
    tr_off = MuZeroTrainer(nets[1], TrainConfig(unroll_steps=K, device_sampling=True), mode="batched",
                           sample_seed=seed)
    # the switch off: the sampled games reanalysed as whole games beforehand
    idx = rp_off.sample_host(B, seed=seed, step=0)["index"]
    rp_off.reanalyse(_reanalyser(nets[1]), games=idx)
    # the targets the two steps are about to assemble
    s = rp_direct.sample(B, seed=seed, step=0)
    np.testing.assert_array_equal(_np(s["index"]), idx)
    n = rp_direct.reanalyse_sample(_reanalyser(nets[2]), s, K)
    got = rp_direct.batch_from(s, K, 0.99)
    want = rp_off.sample_batch(B, K, 0.99, seed=seed, step=0)
    for name in ("obs0", "boot_obs", "acts", "t_rew", "t_pol", "val", "factor", "has_boot"):
        _assert_same_bits(got[name], want[name], name)
    plain = _store(N, trajs, gid0=GID0)
    plain.set_device_priorities(prio)
    assert not torch.equal(got["t_pol"], plain.sample_batch(B, K, 0.99, seed=seed, step=0)["t_pol"])
    # the step
    before = {k: v.clone() for k, v in nets[0].state_dict().items()}
    loss_on = tr_on.train(rp_on, B)
    loss_off = tr_off.train(rp_off, B)
    assert np.isfinite(loss_on) and loss_on == pytest.approx(loss_off, rel=1e-4)
    for k in ("value_loss", "policy_loss", "reward_loss"):
        assert tr_on.last[k] == pytest.approx(tr_off.last[k], rel=1e-4, abs=1e-7)
    assert any(not torch.equal(before[k], v) for k, v in nets[0].state_dict().items())
    assert tr_on.sample_step == 1 and tr_on.last_searched_device.item() == n.item() > 0
    # the step searched the store it trained on: the rows rp_direct holds
    rows = _rows(rp_on)
    for a, b in zip(rows, _rows(rp_direct)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    # reanalyse_every = 2: the second step searches nothing
    assert np.isfinite(tr_on.train(rp_on, B)) and tr_on.sample_step == 2
    for a, b in zip(rows, _rows(rp_on)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    assert tr_on.last_searched_device.item() == n.item()         # (the first step's count still)


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------
def test_refusals():
    import mzgo
    from mzgo import Engine, EngineConfig
    from mzgo._lib import MZGO_EINVAL, MZGO_ENOWEIGHTS, MZGO_OK, lib, ptr, stream_of
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    trajs = _trajs(N)[:2]
    rp = _store(N, trajs, capacity=3)
    dev, A, K = rp.device, N * N + 1, 10
    net = _net(N, C)
    ra = _reanalyser(net)
    items = torch.tensor([[0, 0, 0], [1, 2, 3]], dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    s = stream_of(dev)
    before = _rows(rp)

    def call(handle=rp.handle, eng=ra.engine.handle, it=items, B=2, unroll=K, n=count):
        rc = lib.mzgo_replay_reanalyse_sample(handle, eng, ptr(it), B, unroll, ptr(n), s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    engines = ((Engine(EngineConfig(board_size=N, latent_dim=0, num_games=2)), "board-only"),
               (Engine(EngineConfig(board_size=N, latent_dim=64, num_games=2, num_simulations=4, tower=1,
                                    res_blocks=1)), "tower"),
               (_net(6, 96).engine(2, 4), "board size mismatch (store 5, engine 6)"))
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(eng=None), "null engine"),
                         (dict(it=None), "null items"), (dict(B=0), "B must be >= 1"),
                         (dict(unroll=0), "unroll_steps 0"), (dict(unroll=64), "unroll_steps 64"),
                         *((dict(eng=e.handle), word) for e, word in engines)):
        rc, msg = call(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_reanalyse_sample" in msg and word in msg, (kwargs, rc, msg)
    bare = Engine(EngineConfig(board_size=N, latent_dim=C, num_games=2, num_simulations=4))
    rc, msg = call(eng=bare.handle)
    assert rc == MZGO_ENOWEIGHTS and "missing weight" in msg, (rc, msg)
    for a, b in zip(before, _rows(rp)):                          # a refused call searched nothing
        np.testing.assert_array_equal(a[0], b[0])
    assert call(n=None)[0] == MZGO_OK                            # the count is optional
    assert call()[0] == MZGO_OK and count.item() == len(rp.window_items_host(items, K)) > 0
    with pytest.raises(ValueError, match="6x6"):
        rp.reanalyse_sample(_reanalyser(_net(6, 96)), items, K)
    for bad in (items.cpu(), items.long(), items[:, :2], _np(items)):
        with pytest.raises(ValueError, match="CUDA int32"):
            rp.reanalyse_sample(ra, bad, K)

    # mzgo_replay_batch_items
    out = rp._batch_out(2, K)

    def batch(handle=rp.handle, it=items, B=2, unroll=K, drop=None):
        o = {k: (None if k == drop else ptr(v)) for k, v in out.items()}
        rc = lib.mzgo_replay_batch_items(handle, ptr(it), B, unroll, 0.99, o["obs0"], o["boot_obs"], o["acts"],
                                         o["t_rew"], o["t_pol"], o["val"], o["factor"], o["has_boot"], s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    assert batch()[0] == MZGO_OK
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(it=None), "null items"),
                         (dict(B=0), "B must be >= 1"), (dict(unroll=0), "unroll_steps 0"),
                         (dict(unroll=64), "unroll_steps 64"), (dict(drop="obs0"), "null obs0"),
                         (dict(drop="has_boot"), "null has_boot")):
        rc, msg = batch(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_batch_items" in msg and word in msg, (kwargs, rc, msg)

    # the trainer's constructor
    on = dict(device_sampling=True, reanalyse_sample=True)
    with pytest.raises(ValueError, match="reanalyse_sample needs device_sampling"):
        MuZeroTrainer(net, TrainConfig(reanalyse_sample=True), mode="batched", reanalyser=ra)
    with pytest.raises(ValueError, match="needs a Reanalyser on the trainer's net"):
        MuZeroTrainer(net, TrainConfig(**on), mode="batched")
    with pytest.raises(ValueError, match="needs a Reanalyser on the trainer's net"):
        MuZeroTrainer(net, TrainConfig(**on), mode="batched", reanalyser=_reanalyser(_net(N, C)))
    with pytest.raises(ValueError, match="reanalyse_every must be >= 1"):
        MuZeroTrainer(net, TrainConfig(reanalyse_every=0, **on), mode="batched", reanalyser=ra)
    with pytest.raises(ValueError, match="belong to reanalyse_sample"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True), mode="batched", reanalyser=ra)
    with pytest.raises(ValueError, match="belong to reanalyse_sample"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True, reanalyse_every=2), mode="batched")
    assert MuZeroTrainer(net, TrainConfig(**on), mode="batched", reanalyser=ra).reanalyser is ra
