"""Search-value targets on the CPU: the target rule and the rows it reads,
through their host twins (``mzgo.value_targets_host`` ->
``mzgo_replay_value_targets_host``, ``mzgo.window_items_host(..., td_steps)`` ->
``mzgo_replay_window_items_values_host``: csrc/mzgo_replay.hpp's
``search_value_target`` / ``value_rows`` / ``sample_has``, the kernels' own
functions, run serially), the host target builder under
``TrainConfig.value_target="search"`` and the constructor's refusals.

The rule, restated here in Python float64 (``restated_targets``) without the
library: a game has L moves, rewards r[0..L] (r[L] the winner entry) and root
values nu[0..L-1]; the target of index i with horizon n is the discounted
rewards r[i] .. r[i + n - 1] (stopping after r[L]) plus discount^n times
nu[i + n] if i + n <= L - 1, or times r[L] if i + n == L, rounded to float32
once.  Shared with tests/test_gpu_value_targets.py.
"""
import numpy as np
import pytest
import torch

LENGTHS = [9, 9, 8, 9, 15, 7]                    # test_gpu_replay._trajs(5): the six synthetic games
K_ITEMS = 3


def restated_targets(rewards, root_values, start, K, n, discount):
    """float32 [K + 1]: the rule, read off the formula."""
    L = len(root_values)
    assert len(rewards) == L + 1
    out = []
    for i in range(start, start + K + 1):
        target, factor = 0.0, 1.0
        for j in range(i, i + n):
            if j > L:
                break
            target += factor * float(rewards[j])
            factor *= discount
        if i + n <= L - 1:
            target += factor * float(root_values[i + n])
        elif i + n == L:
            target += factor * float(rewards[L])
        out.append(target)
    return np.array(out, dtype=np.float64).astype(np.float32)


def restated_value_items(length, items, K, n):
    """The item list with value rows: per sample its window and its value
    rows, each row once; by falling t, equal t by batch position."""
    rows = []
    for b, (slot, start, _) in enumerate(np.asarray(items).reshape(-1, 3).tolist()):
        if not 0 <= slot < len(length):
            continue
        L = int(length[slot])
        if L <= 0 or not 0 <= start < L:
            continue
        mine = set(range(start, min(start + K, L - 1) + 1)) | set(range(start + n, min(start + K + n, L - 1) + 1))
        rows += [(t, b, slot) for t in mine]
    rows.sort(key=lambda r: (-r[0], r[1]))
    return np.array([(slot, t) for t, b, slot in rows], np.int32).reshape(-1, 2)


def hand_made_triples(lens):
    """test_hand_made_windows...'s triples: every game but the last from its
    first move, its last and a middle one, then four that contribute nothing."""
    triples = [(k, st, (k + st) % 8) for k, L in enumerate(lens[:-1]) for st in (0, L - 1, L // 2)]
    return triples + [(-1, 0, 0), (len(lens), 0, 0), (0, lens[0], 0), (1, -1, 0)]


def game_values(L, seed):
    """Rewards [L + 1] and root values [L] of mixed sign, a few exactly 0."""
    rng = np.random.default_rng(seed)
    r, nu = rng.uniform(-1.5, 1.5, L + 1), rng.uniform(-1.0, 1.0, L)
    r[rng.integers(0, L + 1, 2)] = 0.0
    nu[rng.integers(0, L, 1)] = 0.0
    return r, nu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
# 1. the target rule's twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 7, 15])
def test_twin_equals_the_rule(L):
    from mzgo import value_targets_host
    r, nu = game_values(L, 40 + L)
    assert (r == 0).any() and (nu == 0).any()
    assert L < 7 or all((x > 0).any() and (x < 0).any() for x in (r, nu))
    seen = set()
    for K in (1, 3, 10):
        for n in sorted({1, K, K + 3, L, L + 5}):
            for discount in (0.99, 1.0):
                for start in range(L):
                    got = value_targets_host(r, nu, start, K, n, discount)
                    want = restated_targets(r, nu, start, K, n, discount)
                    assert got.dtype == np.float32 and got.shape == (K + 1,)
                    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"K {K} n {n} start {start}")
                    seen |= {"searched" if i + n <= L - 1 else "final" if i + n == L else "past"
                             for i in range(start, start + K + 1)}
    assert seen == ({"final", "past"} if L == 1 else {"searched", "final", "past"})


def test_twin_by_hand_and_refusals():
    import ctypes
    from mzgo import value_targets_host
    from mzgo._lib import MZGO_EINVAL, MZGO_OK, lib, ptr
    r, nu = [1.0, 2.0, 4.0, 8.0], [0.5, 0.25, -3.0]              # L = 3
    # n = 2, discount 0.5: i = 0: 1 + 0.5 * 2 + 0.25 * nu[2]; i = 1: 2 + 2 + 0.25 * r[3] (the final board);
    # i = 2: 4 + 0.5 * 8 (nothing past the rewards); i = 3: 8; i = 4: 0
    np.testing.assert_array_equal(value_targets_host(r, nu, 0, 4, 2, 0.5), np.float32([1.25, 6.0, 8.0, 8.0, 0.0]))
    with pytest.raises(ValueError, match="L \\+ 1 rewards"):
        value_targets_host(r, nu[:2], 0, 3, 2, 0.99)
    rr, vv, out = np.array(r), np.array(nu), np.zeros(64, np.float32)

    def call(reward=rr, value=vv, L=3, start=0, K=3, n=2, t_val=out):
        rc = lib.mzgo_replay_value_targets_host(ptr(reward), ptr(value), L, start, K, n, 0.99, ptr(t_val))
        return rc, lib.mzgo_last_error().decode()

    assert call()[0] == MZGO_OK
    for kwargs, word in ((dict(reward=None), "null reward"), (dict(value=None), "null root_value"),
                         (dict(t_val=None), "null t_val"), (dict(L=-1), "L -1"), (dict(start=-1), "start"),
                         (dict(K=0), "unroll_steps 0"), (dict(K=64), "unroll_steps 64"),
                         (dict(n=0), "td_steps must be >= 1"), (dict(n=-2), "td_steps must be >= 1")):
        rc, msg = call(**kwargs)
        assert rc == MZGO_EINVAL and "mzgo_replay_value_targets_host" in msg and word in msg, (kwargs, rc, msg)
    n = ctypes.c_int32()
    items, length, rows = np.array([[0, 0, 0]], np.int32), np.array([5], np.int32), np.zeros((64, 2), np.int32)
    for td in (0, -1):
        rc = lib.mzgo_replay_window_items_values_host(ptr(length), 1, ptr(items), 1, 3, td, ptr(rows), ctypes.byref(n))
        assert rc == MZGO_EINVAL and "td_steps must be >= 1" in lib.mzgo_last_error().decode()
    rc = lib.mzgo_replay_window_items_values_host(None, 1, ptr(items), 1, 3, 2, ptr(rows), ctypes.byref(n))
    assert rc == MZGO_EINVAL and "mzgo_replay_window_items_values_host: null length" in lib.mzgo_last_error().decode()


# ---------------------------------------------------------------------------
# 2. the item list's twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 40])
def test_item_list_twin_equals_the_rule(n):
    from mzgo import window_items_host
    from test_window_items import restated_items
    K, triples = K_ITEMS, hand_made_triples(LENGTHS)
    got = window_items_host(LENGTHS, triples, K, td_steps=n)
    want = restated_value_items(LENGTHS, triples, K, n)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    assert (np.diff(got[:, 1]) <= 0).all() and len(got) <= 2 * len(triples) * (K + 1)
    # without td_steps: today's list, a subset of this one
    plain = window_items_host(LENGTHS, triples, K)
    np.testing.assert_array_equal(plain, window_items_host(LENGTHS, triples, K, td_steps=None))
    np.testing.assert_array_equal(plain, restated_items(LENGTHS, triples, K))
    assert {tuple(r) for r in plain} <= {tuple(r) for r in got}
    # one sample at a time: a gap, a clip at L - 1, no value rows at all
    alone = lambda slot, start: sorted(window_items_host(LENGTHS, [(slot, start, 0)], K, td_steps=n)[:, 1].tolist())
    if n == 5:
        assert alone(4, 0) == [0, 1, 2, 3, 5, 6, 7, 8]          # the 15-move game from 0: rows 0..3 and 5..8
        assert alone(0, 0) == [0, 1, 2, 3, 5, 6, 7, 8]          # 9 moves: value rows 5..8 end exactly at L - 1
        assert alone(4, 7) == [7, 8, 9, 10, 12, 13, 14]         # value rows 12..15 clipped at L - 1 = 14
        assert alone(0, 4) == [4, 5, 6, 7]                      # 4 + 5 > 8: no value rows
    if n == 3:
        assert alone(4, 0) == [0, 1, 2, 3, 4, 5, 6]             # n <= K + 1: one range
    if n == 1:
        assert alone(4, 0) == [0, 1, 2, 3, 4] and alone(0, 8) == [8]
    if n == 40:
        np.testing.assert_array_equal(got, plain)               # no game is that long: the windows alone
    # the dead triples contribute nothing
    for dead in triples[-4:]:
        assert window_items_host(LENGTHS, [dead], K, td_steps=n).shape == (0, 2)


def test_item_list_random_batches():
    from mzgo import window_items_host
    rng = np.random.default_rng(77)
    for cap, B, K, n in ((1, 1, 1, 1), (7, 5, 3, 2), (300, 128, 10, 10), (64, 600, 10, 13), (40, 300, 5, 30)):
        length = rng.integers(0, 41, cap).astype(np.int32)
        items = np.stack([rng.integers(-2, cap + 2, B), rng.integers(-2, 43, B), rng.integers(0, 8, B)], 1)
        got = window_items_host(length, items.astype(np.int32), K, td_steps=n)
        np.testing.assert_array_equal(got, restated_value_items(length, items, K, n))


# ---------------------------------------------------------------------------
# 3. the host builder and the refusals
# ---------------------------------------------------------------------------
def _host_trajs(N=5):
    from oracle.make_golden import synthetic_trajectories
    out = []
    for k, t in enumerate(synthetic_trajectories(N, 6, seed=9)):
        r, nu = game_values(len(t["actions"]), 60 + k)
        out.append(dict(t, rewards=[float(x) for x in r], root_values=[float(x) for x in nu]))
    return out


@pytest.mark.parametrize("K,td", [(3, 0), (3, 5), (10, 1), (10, 13)])
def test_host_builder_under_search(K, td):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    trajs = _host_trajs()
    assert [len(t["actions"]) for t in trajs] == LENGTHS
    net = mzgo.MuZeroNet(32, 26)
    tr = MuZeroTrainer(net, TrainConfig(unroll_steps=K, value_target="search", td_steps=td), mode="batched")
    n = td or K
    assert tr.td_steps == n
    idx = [g for g in range(6) for _ in range(3)]
    starts = [s for L in LENGTHS for s in (0, L - 1, L // 2)]
    batch = [trajs[g] for g in idx]
    obs0, acts, t_val, t_rew, t_pol = tr.host_targets(batch, starts)
    want = np.stack([restated_targets(t["rewards"], t["root_values"], s, K, n, tr.config.discount)
                     for t, s in zip(batch, starts)])
    assert t_val.dtype == torch.float32 and tuple(t_val.shape) == (len(idx), K + 1)
    np.testing.assert_array_equal(_bits(t_val.numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(t_val.numpy()),
                                  _bits(np.stack([mzgo.value_targets_host(t["rewards"], t["root_values"], s, K, n,
                                                                          tr.config.discount)
                                                  for t, s in zip(batch, starts)])))
    # everything else is what the network-target builder gives
    plain = MuZeroTrainer(net, TrainConfig(unroll_steps=K), mode="batched").host_targets(batch, starts)
    for a, b in zip((obs0, acts, t_rew, t_pol), (plain[0], plain[1], plain[3], plain[4])):
        assert torch.equal(a, b)
    assert not torch.equal(t_val, plain[2])
    # a trajectory without root values is named
    bare = {k: v for k, v in trajs[0].items() if k != "root_values"}
    with pytest.raises(ValueError, match="root_values"):
        tr.batch_targets([trajs[1], bare], [0, 0])
    with pytest.raises(ValueError, match="root_values"):
        tr.batch_targets([dict(trajs[0], root_values=trajs[0]["root_values"][:-1])], [0])


def test_default_trainer_builds_network_targets():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig, initial_inference_torch
    c = TrainConfig()
    assert c.value_target == "network" and c.td_steps == 0
    trajs = _host_trajs()
    net = mzgo.MuZeroNet(32, 26)
    net.load_state_dict(mzgo.deterministic_state_dict(32, 26, 3))
    tr = MuZeroTrainer(net, mode="batched")
    assert tr.td_steps is None and tr.config.unroll_steps == 10
    starts = [L // 2 if L < 15 else 1 for L in LENGTHS]         # (only the 15-move game outlasts K = 10)
    got = tr.batch_targets(trajs, starts)
    # main.py's rule (compute_target_value, main.py:503-522), restated: K rewards, then the network's value of the
    # position K moves on where there is one -- evaluated in one batch, in sample-major order, as the builder does
    K, d = 10, c.discount
    want, boots = np.zeros((6, K + 1)), []
    for b, (t, s) in enumerate(zip(trajs, starts)):
        T = len(t["rewards"])
        for k in range(K + 1):
            target, factor = 0.0, 1.0
            for j in range(s + k, min(s + k + K, T)):
                target += factor * t["rewards"][j]
                factor *= d
            want[b, k] = target
            if s + k + K < T:
                boots.append((b, k, factor, t["observations"][s + k + K]))
    assert boots
    with torch.no_grad():
        v = initial_inference_torch(net, torch.as_tensor(np.stack([o for *_, o in boots]), dtype=torch.float32))[1]
    for (b, k, factor, _), vb in zip(boots, v.squeeze(1).numpy()):
        want[b, k] += factor * float(np.float32(vb))
    np.testing.assert_array_equal(got[2].view(np.uint64), want.view(np.uint64))
    # the stored root values play no part in them
    bare = [{k: v for k, v in t.items() if k != "root_values"} for t in trajs]
    for a, b in zip(got, tr.batch_targets(bare, starts)):
        np.testing.assert_array_equal(a, b)
    # and the explicit spelling of the default is the default
    same = MuZeroTrainer(net, TrainConfig(value_target="network", td_steps=0), mode="batched").batch_targets(trajs, starts)
    for a, b in zip(got, same):
        np.testing.assert_array_equal(a, b)


def test_refusals():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="value_target='search' needs mode='batched'"):
        MuZeroTrainer(net, TrainConfig(value_target="search"), mode="reference")
    with pytest.raises(ValueError, match="td_steps belongs to value_target='search'"):
        MuZeroTrainer(net, TrainConfig(td_steps=5), mode="batched")
    with pytest.raises(ValueError, match="td_steps belongs to value_target='search'"):
        MuZeroTrainer(net, TrainConfig(value_target="network", td_steps=10), mode="reference")
    with pytest.raises(ValueError, match="td_steps must be >= 0"):
        MuZeroTrainer(net, TrainConfig(value_target="search", td_steps=-1), mode="batched")
    with pytest.raises(ValueError, match="td_steps must be >= 0"):
        MuZeroTrainer(net, TrainConfig(td_steps=-1), mode="batched")
    with pytest.raises(ValueError, match="value_target must be 'network' or 'search', not 'mcts'"):
        MuZeroTrainer(net, TrainConfig(value_target="mcts"), mode="batched")
    assert MuZeroTrainer(net, TrainConfig(value_target="search"), mode="batched").td_steps == 10
    assert MuZeroTrainer(net, TrainConfig(value_target="search", td_steps=4, unroll_steps=7), mode="batched").td_steps == 4
    assert MuZeroTrainer(net, TrainConfig(), mode="reference").td_steps is None
