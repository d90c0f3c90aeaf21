"""The store's item list on the GPU: ``DeviceReplay.items`` (mzgo_replay_items)
on a wrapped ring, the batch assembly on items no caller should send
(k_replay_batch reads no row outside the store and says what it writes
instead), and the host-index trainer step building its items once.  5x5,
max_moves 12, a ring of 3 slots that took 5 games; C = 16 for the step.
"""
import itertools

import numpy as np
import pytest
import torch

import mzgo
from oracle.make_golden import synthetic_trajectories

pytestmark = pytest.mark.gpu

N, M, CAP = 5, 12, 3
A = N * N + 1


def _games():
    """Five finished 5x5 games of 9, 9, 8, 9 and 7 moves with planted root values."""
    out = []
    for i, t in enumerate(g for g in synthetic_trajectories(N, 6, seed=9) if len(g["actions"]) <= M):
        T = len(t["actions"])
        obs = [o.copy() for o in t["observations"]]
        for o in obs[T:]:
            o[5] = 1.0                                      # the game ended: it has ownership targets
        out.append(dict(t, observations=obs, root_values=[((7 * i + 3 * j) % 11 - 5) / 8.0 for j in range(T)]))
    assert [len(t["actions"]) for t in out] == [9, 9, 8, 9, 7]
    return out


def _wrapped_store():
    rp = mzgo.DeviceReplay(N, CAP, M, "cuda")
    for t in _games():
        rp.add(t)
    slots, length, head = rp._slot_order()
    assert head == 2 and list(slots) == [2, 0, 1] and rp.lengths == [8, 9, 7]
    return rp


def _same(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert torch.equal(got.reshape(-1).contiguous().view(torch.uint8),
                       want.reshape(-1).contiguous().view(torch.uint8)), name


# ---------------------------------------------------------------------------
# 1. items on a wrapped ring
# ---------------------------------------------------------------------------
def test_items_on_a_wrapped_ring():
    rp = _wrapped_store()
    slots = rp._slot_order()[0]
    idx, starts, syms = [0, 2, 1, 2], [0, 6, 8, 3], [3, 0, 7, 4]
    for sy in (None, syms):
        items = rp.items(idx, starts, sy)
        assert items.is_cuda and items.dtype == torch.int32 and tuple(items.shape) == (4, 3)
        want = [[int(slots[g]), s, 0 if sy is None else sy[b]] for b, (g, s) in enumerate(zip(idx, starts))]
        assert items.cpu().tolist() == want
        for K in (1, 3):
            got, ref = rp.batch_from(items, K, 0.99), rp.batch(idx, starts, K, 0.99, sy)
            assert list(got) == list(ref) == ["obs0", "boot_obs", "acts", "t_rew", "t_pol", "val", "factor", "has_boot"]
            for k in ref:
                _same(got[k], ref[k], (k, K))
            got, ref = rp.batch_values_from(items, K, 2, 0.99), rp.batch_values(idx, starts, K, 2, 0.99, sy)
            for k in ref:
                _same(got[k], ref[k], (k, K))
    with pytest.raises(ValueError):
        rp.items([0, 1], [0])
    with pytest.raises(mzgo.MzgoError, match="mzgo_replay_items: sample 1: game 3 is not in the store"):
        rp.items([0, 3], [0, 0])


# ---------------------------------------------------------------------------
# 2. k_replay_batch with items nobody should send
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("search", [False, True], ids=["network", "search"])
def test_batch_assembly_reads_nothing_outside_the_store(search):
    rp = _wrapped_store()
    K, h, L = 2, 1, 7                                       # slot 1 holds the game of 7 moves
    assert rp._slot_order()[1][h] == L
    dev = rp.device
    bad = torch.tensor([[-1, 0, 0], [CAP, 1, 3], [h, -2, 0], [h, L + 5, 5]], dtype=torch.int32, device=dev)
    good = torch.tensor([[h, 0, 0], [h, 1, 0]], dtype=torch.int32, device=dev)
    assemble = (lambda it: rp.batch_values_from(it, K, 2, 0.99)) if search else (lambda it: rp.batch_from(it, K, 0.99))
    got, ref = assemble(bad), assemble(good)
    torch.cuda.synchronize()
    uniform = torch.full((A,), np.float32(1.0 / A), device=dev)
    zeros = torch.zeros(6, N, N, device=dev)
    # a slot outside the ring and a start past the game: an empty game's outputs
    for b in (0, 1, 3):
        _same(got["obs0"][b], zeros, ("obs0", b))
        assert (got["acts"][b] == A - 1).all() and (got["t_rew"][b] == 0).all(), b
        for k in range(K + 1):
            _same(got["t_pol"][b, k], uniform, ("t_pol", b, k))
        if search:
            assert (got["t_val"][b] == 0).all(), b
        else:
            assert (got["boot_obs"][b] == 0).all() and (got["val"][b] == 0).all(), b
            assert (got["factor"][b] == 1).all() and (got["has_boot"][b] == 0).all(), b
    # a held game from start -2: rows -2 and -1 are an empty game's, row 0 is the game's first
    _same(got["obs0"][2], zeros, "obs0")
    assert (got["acts"][2] == A - 1).all() and (got["t_rew"][2] == 0).all()
    for k in (0, 1):
        _same(got["t_pol"][2, k], uniform, ("t_pol", k))
    _same(got["t_pol"][2, 2], ref["t_pol"][0, 0], "t_pol")
    if search:
        assert (got["t_val"][2, :2] == 0).all()
        _same(got["t_val"][2, 2], ref["t_val"][0, 0], "t_val")
    else:
        assert (got["val"][2, :2] == 0).all() and (got["factor"][2, :2] == 1).all()
        for name in ("val", "factor", "has_boot"):
            _same(got[name][2, 2], ref[name][0, 0], name)
        # the bootstrap row of step k is position -2 + k + K = k: inside the game, the game's own boards
        assert (got["has_boot"][2] == 1).all()
        _same(got["boot_obs"][2, 0], ref["obs0"][0], "boot_obs 0")
        _same(got["boot_obs"][2, 1], ref["obs0"][1], "boot_obs 1")
        _same(got["boot_obs"][2, 2], ref["boot_obs"][0, 0], "boot_obs 2")
        assert ref["obs0"][0].abs().sum() + ref["obs0"][1].abs().sum() > 0


# ---------------------------------------------------------------------------
# 3. one upload per host-index step
# ---------------------------------------------------------------------------
def test_the_host_index_step_builds_its_items_once():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    C, B, K = 16, 2, 2

    def step(count):
        rp = _wrapped_store()
        rp.sample_indices = lambda n: np.arange(n)          # games 0 and 1, every step
        calls = []
        if count:
            inner = rp.items
            rp.items = lambda *a, **k: calls.append(a) or inner(*a, **k)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 0))
        torch.manual_seed(11)                               # the heads' initial weights
        starts = itertools.cycle([1, 6])
        tr = MuZeroTrainer(net, TrainConfig(learning_rate=1e-3, unroll_steps=K, fused_loss=True, fused_unroll=True,
                                            value_target="search", ownership_loss_weight=0.25,
                                            consistency_loss_weight=0.5),
                           mode="batched", start_index=lambda T: next(starts))
        loss = tr.train(rp, B)
        return loss, dict(tr.last), len(calls)

    loss, last, n = step(count=True)
    assert n == 1
    assert np.isfinite(loss) and last["ownership_loss"] > 0 and last["consistency_loss"] > 0
    plain_loss, plain_last, _ = step(count=False)
    assert loss == plain_loss and last == plain_last
