"""Search-value targets on the GPU (mzgo.DeviceReplay ``batch_values`` /
``batch_values_from`` / ``sample_batch_values`` / ``reanalyse_sample(...,
td_steps)``; csrc/mzgo_replay.hip: k_replay_batch<true>,
k_replay_window_items<true>) and ``TrainConfig.value_target="search"``.

Everything is compared bit for bit: ``t_val`` with the rule's host twin and
with a Python restatement (tests/test_value_targets.py), the other four
tensors with ``batch()``'s, the searched rows with whole-game reanalysis'.
The loss of a whole step is held to test_gpu_replay's bar for one (rel 1e-4).
test_gpu_replay's shapes: 5x5, C = 96, 16 simulations, four tree slots, the six
synthetic games of 9, 9, 8, 9, 15 and 7 moves.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_reanalyse_sample import GID0, _reanalyser, _rows, _whole_games
from test_gpu_replay import _assert_same_bits, _net, _starts, _store, _trajs
from test_value_targets import (LENGTHS, game_values, hand_made_triples, restated_targets,
                                restated_value_items)

pytestmark = pytest.mark.gpu

N, C = 5, 96
DISCOUNT = 0.99


def _np(t):
    return t.cpu().numpy()


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _valued():
    """The six games with hand-made rewards and root values (mixed sign, a few
    exactly 0): made once, never changed."""
    out = []
    for k, t in enumerate(_trajs(N)):
        r, nu = game_values(len(t["actions"]), 60 + k)
        out.append(dict(t, rewards=[float(x) for x in r], root_values=[float(x) for x in nu]))
    assert [len(t["actions"]) for t in out] == LENGTHS
    return tuple(out)


def _host_t_val(games, idx, starts, K, n):
    import mzgo
    got = np.stack([mzgo.value_targets_host(games[g]["rewards"], games[g]["root_values"], s, K, n, DISCOUNT)
                    for g, s in zip(idx, starts)])
    want = np.stack([restated_targets(games[g]["rewards"], games[g]["root_values"], s, K, n, DISCOUNT)
                     for g, s in zip(idx, starts)])
    np.testing.assert_array_equal(_u32(got), _u32(want))
    return got


# ---------------------------------------------------------------------------
# 1. batch_values against the twin and against batch()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 10])
def test_batch_values_equals_the_twin_and_batch(K):
    trajs = _valued()
    rp = _store(N, trajs, capacity=4)                            # the ring has wrapped: games 2..5 in slots 2, 3, 0, 1
    held = trajs[2:]
    assert len(rp) == 4 and rp.lengths == LENGTHS[2:]
    idx0, st0 = _starts(held)
    idx, starts = idx0 * 8, st0 * 8
    syms = [s for s in range(8) for _ in idx0]                   # every sample under every symmetry
    want = rp.batch(idx, starts, K, DISCOUNT, syms)
    seen = set()
    for n in (1, K, K + 3):
        got = rp.batch_values(idx, starts, K, n, DISCOUNT, syms)
        assert set(got) == {"obs0", "acts", "t_rew", "t_pol", "t_val"}
        assert got["t_val"].dtype == torch.float32 and tuple(got["t_val"].shape) == (len(idx), K + 1)
        np.testing.assert_array_equal(_u32(_np(got["t_val"])), _u32(_host_t_val(held, idx, starts, K, n)), err_msg=f"n {n}")
        for name in ("obs0", "acts", "t_rew", "t_pol"):
            _assert_same_bits(got[name], want[name], name)
        for name, g in rp.batch_values(idx, starts, K, n, DISCOUNT, syms).items():     # a repeat: the same bits
            _assert_same_bits(g, got[name], name)
        for g, s in zip(idx0, st0):
            L = len(held[g]["actions"])
            seen |= {"searched" if s + k + n <= L - 1 else "final" if s + k + n == L else "past" for k in range(K + 1)}
    assert seen == {"searched", "final", "past"}
    # without symmetries: the identity
    plain = rp.batch_values(idx0, st0, K, K, DISCOUNT)
    for name, g in rp.batch_values(idx0, st0, K, K, DISCOUNT, [0] * len(idx0)).items():
        _assert_same_bits(g, plain[name], name)


# ---------------------------------------------------------------------------
# 2. the new rule tied to the old one
# ---------------------------------------------------------------------------
def test_network_values_as_root_values_give_the_network_targets():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    K = 3
    net = _net(N, C).eval()
    games = []
    for t in _valued():
        L = len(t["actions"])
        obs = torch.as_tensor(np.stack(t["observations"][:L]), dtype=torch.float32, device="cuda")
        with torch.no_grad():
            _, v, _ = net.initial_inference(obs)
        games.append(dict(t, root_values=[float(x) for x in _np(v).reshape(L).astype(np.float32)]))
    rp = _store(N, games)
    idx, starts = _starts(games)
    tr = MuZeroTrainer(net, TrainConfig(unroll_steps=K), mode="batched")
    old = _np(tr.device_targets(rp, idx, starts)[2])              # batch + initial_inference + finish_values
    new = _np(rp.batch_values(idx, starts, K, K, DISCOUNT)["t_val"])
    assert tr.config.discount == DISCOUNT
    restated = np.stack([restated_targets(games[g]["rewards"], games[g]["root_values"], s, K, K, DISCOUNT)
                         for g, s in zip(idx, starts)])
    at = np.array(starts)[:, None] + np.arange(K + 1)[None, :] + K
    L = np.array([LENGTHS[g] for g in idx])[:, None]
    assert (at < L).any() and (at == L).any() and (at > L).any()
    np.testing.assert_array_equal(_u32(new)[at != L], _u32(old)[at != L])
    np.testing.assert_array_equal(_u32(new)[at == L], _u32(restated)[at == L])
    np.testing.assert_array_equal(_u32(new), _u32(restated))
    assert (_u32(new)[at == L] != _u32(old)[at == L]).any()       # the final board: r[L] against its network value


# ---------------------------------------------------------------------------
# 3. the sampling paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("symmetries", [False, True])
def test_sample_batch_values_equals_sample_then_batch_values_from(symmetries):
    trajs = _valued()
    B, K, n = len(trajs), 10, 4
    rp = _store(N, trajs)
    rp.set_device_priorities(np.linspace(0.5, 3.0, B))
    for step in range(2):
        host = rp.sample_host(B, seed=8, step=step, symmetries=symmetries)
        want = rp.sample_batch_values(B, K, n, DISCOUNT, seed=8, step=step, symmetries=symmetries)
        s = rp.sample(B, seed=8, step=step, symmetries=symmetries)
        got = rp.batch_values_from(s, K, n, DISCOUNT)
        assert set(got) == {"obs0", "acts", "t_rew", "t_pol", "t_val"}
        np.testing.assert_array_equal(_np(want["items"]), host["items"])
        np.testing.assert_array_equal(_np(want["index"]), host["index"])
        for name in ("items", "index", "gen", "weight"):
            _assert_same_bits(s[name], want[name], name)
        for name, g in got.items():
            _assert_same_bits(g, want[name], name)
        for name, g in rp.batch_values_from(s["items"], K, n, DISCOUNT).items():       # the items tensor alone
            _assert_same_bits(g, want[name], name)
        items = host["items"]
        np.testing.assert_array_equal(_u32(_np(got["t_val"])),
                                      _u32(_host_t_val(trajs, items[:, 0], items[:, 1], K, n)))   # (slot = game here)
    assert not symmetries or host["items"][:, 2].max() > 0


# ---------------------------------------------------------------------------
# 4. window reanalysis over the rows the value targets read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5])
def test_value_rows_equal_whole_game_reanalysis(n):
    K = 3
    net, ra, before, after = _whole_games()
    trajs = _trajs(N)
    lens = [len(t["actions"]) for t in trajs]
    triples = hand_made_triples(lens)
    items = torch.tensor(triples, dtype=torch.int32, device="cuda")
    rp = _store(N, trajs, gid0=GID0)
    prio, gen = _np(rp.device_priorities()), _np(rp.device_generations())
    count = rp.reanalyse_sample(ra, items, K, td_steps=n)
    assert count.is_cuda and count.dtype == torch.int32 and count.shape == (1,)
    want = rp.window_items_host(triples, K, td_steps=n)
    np.testing.assert_array_equal(want, restated_value_items(rp.lengths, triples, K, n))     # (slot = logical index here)
    assert count.item() == len(want) > len(rp.window_items_host(triples, K))
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
    assert not any(k == len(trajs) - 1 for k, _ in inside)       # the last game keeps every row
    if n == 5:                                                    # the 15-move game from 0: rows 0..3 and 5..8, not 4
        assert {(4, 3), (4, 5), (4, 8)} <= inside and (4, 4) not in inside
    # the batch assembled next reads the searched root values
    live = [tr for tr in triples[:-4]]
    t_val = _np(rp.batch_values_from(torch.tensor(live, dtype=torch.int32, device="cuda"), K, n, DISCOUNT)["t_val"])
    games = [rp.export(k) for k in range(len(trajs))]
    np.testing.assert_array_equal(_u32(t_val), _u32(_host_t_val(games, [s for s, _, _ in live], [st for _, st, _ in live],
                                                                K, n)))


# ---------------------------------------------------------------------------
# 5. a trainer step
# ---------------------------------------------------------------------------
def test_train_step_under_search_equals_the_host_builder():
    from mzgo.trainer import MuZeroTrainer, PrioritizedReplayBuffer, TrainConfig
    B, K, n = 4, 3, 5
    trajs = _valued()
    rp = _store(N, trajs)
    exported = [rp.export(k) for k in range(len(trajs))]
    buf = PrioritizedReplayBuffer(len(trajs))
    for t in exported:
        buf.add(t)
    nets = [_net(N, C), _net(N, C)]
    start = lambda T: T // 3
    cfg = lambda: TrainConfig(unroll_steps=K, value_target="search", td_steps=n)
    tr_h = MuZeroTrainer(nets[0], cfg(), mode="batched", start_index=start)
    tr_d = MuZeroTrainer(nets[1], cfg(), mode="batched", start_index=start)
    np.random.seed(0)
    idx = rp.sample_indices(B)
    starts = [start(rp.lengths[i]) for i in idx]
    want = tr_h.host_targets([exported[i] for i in idx], starts)
    got = tr_d.device_targets(rp, idx, starts)
    for name, a, b in zip(("obs0", "acts", "t_val", "t_rew", "t_pol"), got, want):
        _assert_same_bits(a, b, name)
    np.testing.assert_array_equal(_u32(_np(got[2])), _u32(_host_t_val(trajs, idx, starts, K, n)))
    before = {k: v.clone() for k, v in nets[1].state_dict().items()}
    np.random.seed(0)
    loss_h = tr_h.train(buf, B)
    np.random.seed(0)
    loss_d = tr_d.train(rp, B)
    assert np.isfinite(loss_d) and loss_d == pytest.approx(loss_h, rel=1e-4)
    for k in ("value_loss", "policy_loss", "reward_loss"):
        assert tr_d.last[k] == pytest.approx(tr_h.last[k], rel=1e-4, abs=1e-7)
    assert any(not torch.equal(before[k], v) for k, v in nets[1].state_dict().items())
    # the targets differ from the network's: the step trained on the stored values
    plain = MuZeroTrainer(nets[1], TrainConfig(unroll_steps=K), mode="batched").device_targets(rp, idx, starts)
    assert not torch.equal(plain[2], got[2])


def test_device_sampled_step_with_reanalysis_trains_on_the_searched_values():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    B, K, n, seed = 4, 3, 5, 5
    trajs = _valued()
    rp = _store(N, trajs, gid0=GID0)
    rp.set_device_priorities(np.linspace(0.5, 3.0, len(trajs)))
    net = _net(N, C)
    tr = MuZeroTrainer(net, TrainConfig(unroll_steps=K, value_target="search", td_steps=n, device_sampling=True,
                                        reanalyse_sample=True), mode="batched", sample_seed=seed,
                       reanalyser=_reanalyser(net))
    items = rp.sample_host(B, seed=seed, step=0)["items"]        # the draw the step is about to make
    rows_before = _rows(rp)
    assert np.isfinite(tr.train(rp, B)) and tr.sample_step == 1
    listed = rp.window_items_host(items, K, td_steps=n)
    assert tr.last_searched_device.item() == len(listed) > 0
    rows_after = _rows(rp)
    for k, L in enumerate(LENGTHS):                               # exactly the listed rows were searched
        for row in range(L):
            changed = rows_after[k][1][row] != rows_before[k][1][row] or \
                not np.array_equal(rows_after[k][0][row], rows_before[k][0][row])
            assert changed == ((k, row) in {(int(s), int(t)) for s, t in listed}), (k, row)
    games = [rp.export(k) for k in range(len(trajs))]            # the store's rows after the reanalysis
    want = _host_t_val(games, items[:, 0], items[:, 1], K, n)    # (slot = game here)
    assert tuple(tr.last_t_val_device.shape) == (B, K + 1)
    np.testing.assert_array_equal(_u32(_np(tr.last_t_val_device)), _u32(want))
    stale = _host_t_val(trajs, items[:, 0], items[:, 1], K, n)
    assert (_u32(want) != _u32(stale)).any()                      # some target read a searched value
    # without reanalysis on the step, sample_batch_values serves it
    tr2 = MuZeroTrainer(_net(N, C), TrainConfig(unroll_steps=K, value_target="search", device_sampling=True),
                        mode="batched", sample_seed=seed)
    items2 = rp.sample_host(B, seed=seed, step=0)["items"]
    assert np.isfinite(tr2.train(rp, B)) and tr2.td_steps == K
    np.testing.assert_array_equal(_u32(_np(tr2.last_t_val_device)),
                                  _u32(_host_t_val(games, items2[:, 0], items2[:, 1], K, K)))


# ---------------------------------------------------------------------------
# 6. refusals, through ctypes
# ---------------------------------------------------------------------------
def test_refusals():
    from mzgo._lib import MZGO_EINVAL, MZGO_OK, lib, ptr, stream_of
    trajs = list(_valued()[:2])
    rp = _store(N, trajs, capacity=3)
    dev, K = rp.device, 10
    out = rp._values_out(2, K)
    s = stream_of(dev)
    items = torch.tensor([[0, 0, 0], [1, 2, 3]], dtype=torch.int32, device=dev)
    T0 = len(trajs[0]["actions"])

    # host samples: the samples' checks are mzgo_replay_items', the rest mzgo_replay_batch_items_values' (below)
    up = torch.zeros(2, 3, dtype=torch.int32, device=dev)

    def host(handle=rp.handle, idx=(0, 1), starts=(0, 1), syms=None, B=2, it=up):
        i32 = lambda x: None if x is None else np.array(x, np.int32)
        a, b, c = i32(idx), i32(starts), i32(syms)
        rc = lib.mzgo_replay_items(handle, ptr(a), ptr(b), ptr(c), B, ptr(it), s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    assert host()[0] == MZGO_OK and up.cpu().tolist() == [[0, 0, 0], [1, 1, 0]]
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(B=0), "B must be >= 1"),
                         (dict(idx=None), "null indices"), (dict(starts=None), "null starts"),
                         (dict(it=None), "null items"),
                         (dict(idx=(0, 2)), "game 2 is not in the store"), (dict(idx=(-1, 0)), "game -1"),
                         (dict(starts=(T0, 0)), f"start {T0} outside"), (dict(starts=(0, -1)), "start -1 outside"),
                         (dict(syms=(0, 8)), "symmetry 8")):
        rc, msg = host(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_items" in msg and word in msg, (kwargs, rc, msg)

    def dev_items(handle=rp.handle, it=items, B=2, unroll=K, td=K, drop=None):
        o = {k: (None if k == drop else ptr(v)) for k, v in out.items()}
        rc = lib.mzgo_replay_batch_items_values(handle, ptr(it), B, unroll, td, 0.99, o["obs0"], o["acts"], o["t_rew"],
                                                o["t_pol"], o["t_val"], s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    assert dev_items()[0] == MZGO_OK
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(it=None), "null items"),
                         (dict(B=0), "B must be >= 1"), (dict(unroll=0), "unroll_steps 0"),
                         (dict(unroll=64), "unroll_steps 64"), (dict(td=0), "td_steps must be >= 1"),
                         (dict(td=-3), "td_steps must be >= 1"), (dict(drop="obs0"), "null obs0"),
                         (dict(drop="t_pol"), "null t_pol"), (dict(drop="t_rew"), "null t_rew"),
                         (dict(drop="t_val"), "null t_val")):
        rc, msg = dev_items(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_batch_items_values" in msg and word in msg, (kwargs, rc, msg)

    so = rp._sample_out(2)

    # a sampled batch: the draw's checks are mzgo_replay_sample's, the assembly's are dev_items' above
    def sampled(handle=rp.handle, B=2, beta=0.0, drop=None):
        o = {k: (None if k == drop else ptr(v)) for k, v in so.items()}
        rc = lib.mzgo_replay_sample(handle, B, 1, 0, 0, beta, o["items"], o["index"], o["gen"], o["weight"], s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    assert sampled()[0] == MZGO_OK and dev_items(it=so["items"])[0] == MZGO_OK
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(B=0), "B must be >= 1"), (dict(B=3), "B 3 exceeds"),
                         (dict(beta=-1.0), "beta"), (dict(drop="items"), "null items")):
        rc, msg = sampled(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_sample" in msg and word in msg, (kwargs, rc, msg)

    ra = _reanalyser(_net(N, C))
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    before = _rows(rp)

    def search(handle=rp.handle, eng=ra.engine.handle, it=items, B=2, unroll=K, td=2, n=count):
        rc = lib.mzgo_replay_reanalyse_sample_values(handle, eng, ptr(it), B, unroll, td, ptr(n), s)
        torch.cuda.synchronize()
        return rc, lib.mzgo_last_error().decode()

    six_net = _net(6, 96)
    six = six_net.engine(2, 4)                                   # (held here: a handle does not keep its engine alive)
    for kwargs, word in ((dict(handle=None), "null replay"), (dict(eng=None), "null engine"),
                         (dict(it=None), "null items"), (dict(B=0), "B must be >= 1"),
                         (dict(unroll=0), "unroll_steps 0"), (dict(td=0), "td_steps must be >= 1"),
                         (dict(eng=six.handle), "board size mismatch (store 5, engine 6)")):
        rc, msg = search(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_reanalyse_sample_values" in msg and word in msg, (kwargs, rc, msg)
    for a, b in zip(before, _rows(rp)):                          # a refused call searched nothing
        np.testing.assert_array_equal(a[0], b[0])
    assert search(n=None)[0] == MZGO_OK
    assert search()[0] == MZGO_OK and count.item() == len(rp.window_items_host(items, K, td_steps=2)) > 0
