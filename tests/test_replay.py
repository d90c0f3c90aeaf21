"""The device replay store's host side (mzgo.replay), no GPU needed:

* the symmetry index tables the batch kernel uses (read through
  mzgo_replay_symmetry_table, which runs the kernel's own index functions on
  the host) equal the numpy definition -- rot90 by s & 3, then a flip of the
  last axis if s & 4 -- for planes, policy rows and actions;
* the ledger draws the indices ``PrioritizedReplayBuffer.sample`` draws from
  the same ``np.random`` state, after eviction and after priority updates.
"""
import ctypes

import numpy as np
import pytest


def _transform(x, s):
    y = np.rot90(x, s & 3, axes=(-2, -1))
    return np.flip(y, axis=-1) if s & 4 else y


@pytest.mark.parametrize("N", [5, 6])
@pytest.mark.parametrize("s", range(8))
def test_symmetry_tables_equal_the_numpy_definition(N, s):
    from mzgo.replay import symmetry_tables
    C = N * N
    src, dst = symmetry_tables(N, s)
    assert src.shape == (C,) and dst.shape == (C + 1,)
    assert sorted(src) == list(range(C)) and sorted(dst) == list(range(C + 1))
    rng = np.random.default_rng(100 * N + s)
    planes = rng.random((6, N, N))
    np.testing.assert_array_equal(planes.reshape(6, C)[:, src].reshape(6, N, N), _transform(planes, s))
    pol = rng.random(C + 1)
    want = np.concatenate([_transform(pol[:C].reshape(N, N), s).reshape(-1), pol[C:]])
    np.testing.assert_array_equal(np.concatenate([pol[:C][src], pol[C:]]), want)
    for a in range(C + 1):                       # an action moves where its one-hot would; pass stays
        hot = np.zeros(C + 1)
        hot[a] = 1.0
        moved = np.concatenate([_transform(hot[:C].reshape(N, N), s).reshape(-1), hot[C:]])
        assert int(np.argmax(moved)) == dst[a]
    assert dst[C] == C
    if s == 0:
        assert list(src) == list(range(C))


def test_symmetry_table_refuses_bad_arguments():
    from mzgo import _lib
    buf = np.zeros(400, np.int32)
    for N, s in ((1, 0), (20, 0), (5, 8), (5, -1)):
        rc = _lib.lib.mzgo_replay_symmetry_table(N, s, _lib.ptr(buf), _lib.ptr(buf))
        assert rc == _lib.MZGO_EINVAL
        assert b"mzgo_replay_symmetry_table" in _lib.lib.mzgo_last_error()


def test_replay_create_refuses_bad_arguments():
    from mzgo import _lib
    h = ctypes.c_void_p()
    for args, word in (((1, 4, 10, 0), b"board_size"), ((5, 0, 10, 0), b"capacity"), ((5, 4, 0, 0), b"max_moves")):
        rc = _lib.lib.mzgo_replay_create(*args, ctypes.byref(h))
        assert rc == _lib.MZGO_EINVAL and not h.value
        assert word in _lib.lib.mzgo_last_error()
    assert _lib.lib.mzgo_replay_create(5, 4, 10, 0, None) == _lib.MZGO_EINVAL


def test_ledger_samples_what_the_prioritized_buffer_samples():
    from mzgo.replay import ReplayLedger
    from mzgo.trainer import PrioritizedReplayBuffer
    cap = 6
    led, buf = ReplayLedger(cap), PrioritizedReplayBuffer(cap)
    for g in range(9):                           # three past the capacity: games 0..2 are evicted
        led.push(4 + g, 100 + g)
        buf.add({"id": g})
    assert len(led) == cap and led.lengths == [7, 8, 9, 10, 11, 12] and led.key_gids == list(range(103, 109))
    assert led.priorities == buf.priorities == [1.0] * cap
    for seed, n in ((0, 3), (1, 6), (2, 1)):
        np.random.seed(seed)
        want = buf.sample(n)[1]
        np.random.seed(seed)
        got = led.sample_indices(n)
        np.testing.assert_array_equal(got, want)
    led.update_priorities([0, 3, 5], [0.25, 7.5, 1e-3])
    buf.update_priorities([0, 3, 5], [0.25, 7.5, 1e-3])
    assert led.priorities == buf.priorities
    led.push(5, 1)                               # eviction shifts the priorities with the games
    buf.add({"id": 9})
    assert led.priorities == buf.priorities == [1.0, 1.0, 7.5, 1.0, 1e-3, 1.0]
    np.random.seed(5)
    picks, want = buf.sample(4)
    after_buf = np.random.random()
    np.random.seed(5)
    got = led.sample_indices(4)
    after_led = np.random.random()
    np.testing.assert_array_equal(got, want)
    assert [p["id"] for p in picks] == [4 + i for i in got]
    assert after_led == after_buf                # the same draws: the np.random stream stays main.py's


def test_trainer_config_symmetries_default_off():
    from mzgo.trainer import TrainConfig
    assert TrainConfig().symmetries is False
