"""The device priority ledger and sampler on the GPU (mzgo.DeviceReplay
``sample`` / ``sample_batch`` / ``update_device_priorities``;
csrc/mzgo_replay.hip: k_replay_sample_build, k_replay_sample_draw,
k_replay_update_priorities, k_replay_new_games) and ``TrainConfig.device_sampling``.

The sampler's kernels are compared bit for bit with the host twin, which
tests/test_replay_sample.py compares with an independent restatement; the
stores here are 2x2 boards with games of 0..3 moves added through ``add``, so
that a 5000-slot store is small.  A whole trainer step is compared with
``_unroll_step`` on the same sampled values under test_gpu_replay's bar (loss
and parts rel 1e-4), parameter gradients under test_loss's (rtol 1e-3, atol
1e-5 max |ref|: MIOpen's backward may add in another order from run to run).
"""
import functools

import numpy as np
import pytest
import torch

from test_replay_sample import FLT_MIN, build_case

pytestmark = pytest.mark.gpu

K = 10


def _tiny_game(T, k):
    """A 2x2 'game' of T moves in main.py's format (what it shows does not
    matter to the sampler: stones alternate, policies are uniform)."""
    obs = []
    for t in range(T + 1):
        o = np.zeros((6, 2, 2))
        o[t % 2].flat[(t + k) % 4] = 1.0
        o[2] = t % 2
        obs.append(o)
    return dict(observations=obs + [obs[-1]], actions=[(t + k) % 5 for t in range(T)], rewards=[0.0] * T + [1.0],
                policies=[np.full(5, 0.2)] * T)


@functools.lru_cache(maxsize=None)
def _store(cap):
    """A store whose slots hold test_replay_sample.build_case(cap): cap + head
    adds (game k lands in slot k % cap, so the ring ends wrapped at ``head``
    with the first ``head`` slots written twice), then the case's weights."""
    import mzgo
    prio, length, head = build_case(cap)
    rp = mzgo.DeviceReplay(2, cap, 3, "cuda")
    for k in range(cap + head):
        rp.add(_tiny_game(int(length[k % cap]), k))
    assert len(rp) == cap
    rp.set_device_priorities(prio[(head + np.arange(cap)) % cap])
    return rp


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("cap", [1, 64, 65, 4097, 5000])
def test_kernel_equals_the_twin(cap):
    from mzgo.replay import sample_host
    prio, length, head = build_case(cap)
    rp = _store(cap)
    n_valid = int((length > 0).sum())
    np.testing.assert_array_equal(_np(rp.device_priorities()), prio[(head + np.arange(cap)) % cap])
    want_gen = 1 + (np.arange(cap) < head)
    np.testing.assert_array_equal(_np(rp.device_generations()), want_gen[(head + np.arange(cap)) % cap])
    for B, sym, beta in ((1, False, 0.0), (min(n_valid, 128), True, 0.5)):
        step = 10 * cap + B
        got = rp.sample(B, seed=21, step=step, symmetries=sym, beta=beta)
        want = sample_host(prio, length, head, B, seed=21, step=step, symmetries=sym, beta=beta)
        np.testing.assert_array_equal(_np(got["index"]), want["index"])
        np.testing.assert_array_equal(_np(got["items"]), want["items"])
        np.testing.assert_array_equal(_np(got["gen"]), want_gen[want["items"][:, 0]])
        np.testing.assert_allclose(_np(got["weight"]).astype(np.float64), want["weight"].astype(np.float64),
                                   rtol=1e-6)
        assert _np(got["weight"]).max() == 1.0
        again = rp.sample(B, seed=21, step=step, symmetries=sym, beta=beta)
        for k in ("index", "items", "gen", "weight"):
            assert torch.equal(got[k], again[k]), k
        mine = rp.sample_host(B, seed=21, step=step, symmetries=sym, beta=beta)
        np.testing.assert_array_equal(mine["items"], want["items"])
        if n_valid > B > 1:                          # (one draw mostly finds the heaviest game)
            other = rp.sample(B, seed=21, step=step + 1, symmetries=sym, beta=beta)
            assert not torch.equal(got["items"], other["items"])
    if cap >= 64:
        assert head != 0 and (length == 0).any() and prio.min() == FLT_MIN and prio.max() == 1e3


@pytest.mark.parametrize("N,B", [(5, 6), (9, 2)])
@pytest.mark.parametrize("symmetries", [False, True])
def test_sample_batch_equals_batch(N, B, symmetries):
    from test_gpu_replay import _assert_same_bits, _store as game_store, _trajs
    trajs = _trajs(N, B)
    rp = game_store(N, trajs)
    rp.set_device_priorities(np.linspace(0.5, 3.0, B))
    for step in range(3):
        s = rp.sample_batch(B, K, 0.99, seed=8, step=step, symmetries=symmetries)
        items = _np(s["items"])
        idx, starts, syms = _np(s["index"]), items[:, 1], items[:, 2]
        assert sorted(idx.tolist()) == list(range(B)) and (items[:, 0] == idx).all()
        assert all(0 <= st < len(trajs[i]["actions"]) for i, st in zip(idx, starts))
        assert (syms == 0).all() if not symmetries else ((syms >= 0) & (syms < 8)).all()
        want = rp.batch(idx, starts, K, 0.99, syms if symmetries else None)
        for name, w in want.items():
            _assert_same_bits(s[name], w, name)
    assert not symmetries or len({tuple(_np(rp.sample(B, seed=8, step=t, symmetries=True)["items"])[:, 2])
                                  for t in range(4)}) > 1


def _small(n=8, cap=8):
    import mzgo
    rp = mzgo.DeviceReplay(2, cap, 3, "cuda")
    for k in range(n):
        rp.add(_tiny_game(1 + k % 3, k))
    return rp


def test_priority_update():
    rp = _small()
    s = rp.sample(6, seed=1, step=0)
    idx = _np(s["index"])
    tiny32 = np.float32(1e-45)                                          # a float32 denormal: floored
    per = np.array([0.5, 0.0, np.nan, -1.0, 3.0, tiny32], np.float32)
    rp.update_device_priorities(s, torch.from_numpy(per).cuda())
    want = np.ones(8)
    for i, p in zip(idx, per):
        if np.isfinite(p) and p >= 0:
            want[i] = max(float(p), FLT_MIN)
    got = _np(rp.device_priorities())
    np.testing.assert_array_equal(got, want)                            # exact at alpha = 1
    assert got[idx[1]] == FLT_MIN and got[idx[5]] == FLT_MIN and got[idx[2]] == 1.0 and got[idx[3]] == 1.0
    assert rp.skipped_updates() == 2
    # alpha
    per = np.array([0.5, 0.0, 7.25, 1e-3, 3.0, 123.0], np.float32)
    rp.update_device_priorities(s, torch.from_numpy(per).cuda(), alpha=0.7)
    want = np.ones(8)
    want[idx] = np.maximum(per.astype(np.float64), FLT_MIN) ** 0.7
    np.testing.assert_allclose(_np(rp.device_priorities()), want, rtol=1e-12)
    assert rp.skipped_updates() == 2
    # the batch-mean mode: one device scalar for all B
    mean = torch.tensor([2.625], dtype=torch.float64, device="cuda")
    rp.update_device_priorities(s, mean=mean)
    want[idx] = 2.625
    np.testing.assert_array_equal(_np(rp.device_priorities()), want)
    rp.update_device_priorities(s, mean=mean * float("inf"))
    np.testing.assert_array_equal(_np(rp.device_priorities()), want)
    assert rp.skipped_updates() == 2 + 6
    with pytest.raises(ValueError):
        rp.update_device_priorities(s)


def test_generation_guard():
    rp = _small()
    s = rp.sample(8, seed=2, step=0)                                    # every game, slots 0 and 1 among them
    assert sorted(_np(s["index"]).tolist()) == list(range(8))
    rp.add(_tiny_game(2, 100))                                          # evicts logical 0 = slot 0
    rp.add(_tiny_game(3, 101))                                          # ... and slot 1
    per = torch.arange(2.0, 10.0, device="cuda")
    rp.update_device_priorities(s, per)
    got = _np(rp.device_priorities())                                   # logical i is slot (2 + i) % 8
    slot_loss = np.empty(8)
    slot_loss[_np(s["items"])[:, 0]] = _np(per)
    np.testing.assert_array_equal(got[:6], slot_loss[2:])
    np.testing.assert_array_equal(got[6:], [1.0, 1.0])
    np.testing.assert_array_equal(_np(rp.device_generations()), [1] * 6 + [2, 2])
    assert rp.skipped_updates() == 0


def test_new_games_from_an_engine():
    import mzgo
    from mzgo.trainer import MainSelfPlay
    from test_gpu_replay import _net
    N, C, G = 5, 96, 4
    msp = MainSelfPlay(_net(N, C, 5).eval(), G, 4, seed=3)
    rp = mzgo.DeviceReplay(N, 8, msp.max_moves, "cuda")
    msp.play_into(rp)                                                   # add_games
    np.testing.assert_array_equal(_np(rp.device_priorities()), [1.0] * 4)
    np.testing.assert_array_equal(_np(rp.device_generations()), [1] * 4)
    rp.set_device_priorities([2.0, 3.0, 4.0, 5.0])
    msp.play_games_into(rp, 6)                                          # slots 4..7, then 0 and 1 again
    assert len(rp) == 8
    np.testing.assert_array_equal(_np(rp.device_priorities()), [4.0, 5.0] + [1.0] * 6)
    np.testing.assert_array_equal(_np(rp.device_generations()), [1] * 6 + [2, 2])
    assert rp.priorities == [1.0] * 8                                   # the host ledger is its own


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
def _trainer_setup(n_games=10):
    from test_gpu_replay import _store as game_store, _trajs
    N = 5
    rp = game_store(N, _trajs(N, n_games))
    rp.set_device_priorities(np.linspace(0.5, 4.0, n_games))
    return N, 96, rp


@pytest.mark.parametrize("fused", [False, True])
def test_train_step_with_device_sampling(fused):
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from test_gpu_replay import _net
    N, C, rp = _trainer_setup()
    B, K3 = 8, 3
    before = _np(rp.device_priorities())
    s = rp.sample(B, seed=5, step=0)                                    # the sample the step is about to draw
    idx, starts = _np(s["index"]), _np(s["items"])[:, 1]
    tr_d = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=K3, device_sampling=True, sample_priorities=True,
                                                 fused_loss=fused), mode="batched", sample_seed=5)
    tr_r = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=K3, fused_loss=fused), mode="batched")
    loss_r = tr_r._unroll_step(*tr_r.device_targets(rp, idx, starts), device_totals=True)
    loss_d = tr_d.train(rp, B)
    assert isinstance(loss_d, float) and np.isfinite(loss_d) and loss_d == pytest.approx(loss_r, rel=1e-4)
    for k in ("value_loss", "policy_loss", "reward_loss"):
        assert tr_d.last[k] == pytest.approx(tr_r.last[k], rel=1e-4, abs=1e-7)
    assert tr_d.sample_step == 1 and tr_d.scheduler.last_epoch == 1
    for a, b in zip(tr_d.net.parameters(), tr_r.net.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5)
    # the priorities afterwards are the per-sample losses
    per = _np(tr_d.last_per_sample_device).astype(np.float64)
    assert per.shape == (B,) and per.sum() / B == pytest.approx(loss_d, rel=1e-5)
    want = before.copy()
    want[idx] = np.maximum(per, FLT_MIN)
    np.testing.assert_array_equal(_np(rp.device_priorities()), want)
    assert rp.priorities == [1.0] * len(rp)                             # the host ledger was not touched
    # sample_priorities off: the batch mean for every sampled game
    tr_m = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=K3, device_sampling=True, fused_loss=fused),
                         mode="batched", sample_seed=6)
    idx_m = _np(rp.sample(B, seed=6, step=0)["index"])
    loss_m = tr_m.train(rp, B)
    got = _np(rp.device_priorities())
    assert (got[idx_m] == loss_m).all()
    assert tr_m.train(rp, len(rp) + 1) is None


@pytest.mark.parametrize("fused", [False, True])
def test_importance_weighted_gradient(fused):
    import torch.nn.functional as F
    from mzgo.trainer import (MuZeroTrainer, TrainConfig, initial_inference_torch, recurrent_inference_torch)
    from test_gpu_replay import _net
    N, C, rp = _trainer_setup()
    B, K3 = 8, 3
    cfg = TrainConfig(unroll_steps=K3, learning_rate=0.0, max_grad_norm=1e9, device_sampling=True,
                      importance_beta=0.5, fused_loss=fused)
    tr = MuZeroTrainer(_net(N, C), cfg, mode="batched", sample_seed=9)
    s = rp.sample(B, seed=9, step=0, beta=0.5)
    w = s["weight"]
    assert w.max().item() == 1.0 and w.min().item() < 0.9
    idx, starts = _np(s["index"]), _np(s["items"])[:, 1]
    loss = tr.train(rp, B)
    # the weighted torch expression on a copy of the net
    ref = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=K3), mode="batched")
    obs0, acts, t_val, t_rew, t_pol = ref.device_targets(rp, idx, starts)
    kl = lambda lg, tp: F.kl_div(F.log_softmax(lg, dim=1), tp, reduction="none").sum(dim=1)
    latent, value, logits = initial_inference_torch(ref.net, obs0)
    per = ref._value_loss(value.squeeze(1), t_val[:, 0]) + kl(logits, t_pol[:, 0])
    for k in range(1, K3 + 1):
        latent, reward, value, logits = recurrent_inference_torch(ref.net, latent, acts[:, k - 1])
        per = per + F.mse_loss(reward.squeeze(1), t_rew[:, k - 1], reduction="none") \
            + ref._value_loss(value.squeeze(1), t_val[:, k]) + kl(logits, t_pol[:, k])
    ref.net.zero_grad()
    (per * w).sum().backward()
    assert loss == pytest.approx(per.sum().item() / B, rel=1e-4)        # the reported loss stays unweighted
    for (name, a), b in zip(tr.net.named_parameters(), ref.net.parameters()):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-3, atol=1e-5 * max(1.0, b.grad.abs().max().item()),
                                   msg=lambda m: f"{name}: {m}")
        assert torch.equal(a.detach(), b.detach())                      # learning rate 0
    # the priorities are the unweighted mean
    assert (_np(rp.device_priorities())[idx] == loss).all()


def test_deferred_stats():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from test_gpu_replay import _net
    N, C, rp = _trainer_setup()
    tr = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=3, device_sampling=True, deferred_stats=True,
                                               fused_loss=True, sample_priorities=True), mode="batched")
    out = tr.train(rp, 8)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dim() == 0 and out.dtype == torch.float64
    assert tr.last == {}
    stats = tr.read_stats()
    assert out.item() == stats["training_loss"] and set(stats) == {"training_loss", "value_loss", "policy_loss",
                                                                    "reward_loss", "lr"}
    assert tr.read_stats() is stats and tr.last is stats


def test_refusals():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, PrioritizedReplayBuffer, TrainConfig
    rp = _small(5, 8)
    rp.add(_tiny_game(0, 9))                                            # a game without moves weighs nothing
    with pytest.raises(mzgo.MzgoError, match="exceeds the 5 stored games"):
        rp.sample(6, seed=1, step=0)
    assert sorted(_np(rp.sample(5, seed=1, step=0)["index"]).tolist()) == [0, 1, 2, 3, 4]
    with pytest.raises(mzgo.MzgoError, match="B must be >= 1"):
        rp.sample(0, seed=1, step=0)
    with pytest.raises(mzgo.MzgoError, match="unroll_steps 0"):
        rp.sample_batch(2, 0, 0.99, seed=1, step=0)
    for bad in ([1.0] * 5 + [0.0], [1.0] * 5 + [float("nan")], [1.0] * 5 + [float("inf")], [1.0] * 5):
        with pytest.raises(mzgo.MzgoError, match="mzgo_replay_set_priorities"):
            rp.set_device_priorities(bad)
    big = mzgo.DeviceReplay(2, 64 ** 3 + 1, 1, "cuda")                  # the store itself has no such limit
    big.add(_tiny_game(1, 0))
    with pytest.raises(mzgo.MzgoError, match=r"64\^3"):
        big.sample(1, seed=1, step=0)
    big.close()
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="device_sampling"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True), mode="reference")
    with pytest.raises(ValueError, match="DeviceReplay"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True), mode="batched").train(PrioritizedReplayBuffer(4), 2)
