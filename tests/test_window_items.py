"""The window rule of a sampled batch on the CPU, through its host twin
(``mzgo.replay.window_items_host`` -> ``mzgo_replay_window_items_host``, which
runs csrc/mzgo_replay.hpp's ``window_rows`` / ``window_has`` -- the builder
kernel's own functions -- serially).

A sample (slot, start, symmetry) under K unroll steps on a game of L moves
reads the stored policy rows t = start .. min(start + K, L - 1); a slot outside
the store, an empty game or a start outside 0 .. L - 1 contributes nothing.
The item list is every (slot, t) by falling t, equal t by batch position.
``restated_items`` says that with a Python sort; the twin must give the same
rows in the same order.  Shared with tests/test_gpu_reanalyse_sample.py.
"""
import numpy as np
import pytest

# slot:     0  1  2  3   4   5
LENGTHS = [0, 1, 5, 12, 30, 2]
# (slot, start, symmetry): an empty game; a game of one move; a window that
# clips at L - 1 for every K (slot 2 from 3) and one that clips for none (slot
# 4 from 2: 2 + 10 < 29); the same t from several samples (the tie goes to the
# earlier one); a slot drawn twice; slots and starts out of range
ITEMS = [(4, 2, 0), (0, 0, 1), (2, 3, 2), (1, 0, 3), (3, 3, 4), (4, 3, 5), (2, 0, 6), (5, 1, 7),
         (-1, 0, 0), (6, 0, 0), (3, -1, 0), (3, 12, 0), (2, 5, 0), (1, 1, 0), (3, 11, 0), (4, 29, 0),
         (2 ** 31 - 1, 0, 0), (4, 2 ** 31 - 1, 0), (-2 ** 31, 0, 0), (4, -2 ** 31, 0)]


def restated_items(length, items, K):
    rows = []
    for b, (slot, start, _) in enumerate(np.asarray(items).reshape(-1, 3).tolist()):
        if not 0 <= slot < len(length):
            continue
        L = int(length[slot])
        if L <= 0 or not 0 <= start < L:
            continue
        rows += [(t, b, slot) for t in range(start, min(start + K, L - 1) + 1)]
    rows.sort(key=lambda r: (-r[0], r[1]))
    return np.array([(slot, t) for t, b, slot in rows], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("K", [1, 3, 10])
def test_twin_equals_the_rule(K):
    from mzgo.replay import window_items_host
    got = window_items_host(LENGTHS, ITEMS, K)
    want = restated_items(LENGTHS, ITEMS, K)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    # the count, said once more by hand: min(K, L - 1 - start) + 1 rows per live sample
    live = [(4, 2), (2, 3), (1, 0), (3, 3), (4, 3), (2, 0), (5, 1), (3, 11), (4, 29)]
    assert len(got) == sum(min(K, LENGTHS[s] - 1 - st) + 1 for s, st in live) > 0
    # latest first, ties in batch order: slot 4's t = 3 (sample 0) before slot 3's (sample 4) before slot 4's (sample 5)
    at3 = [tuple(r) for r in got if r[1] == 3 and r[0] in (3, 4)]
    assert at3[:3] == [(4, 3), (3, 3), (4, 3)]
    assert (np.diff(got[:, 1]) <= 0).all()
    # slot 2 from 3 stops at L - 1 = 4; slot 4 from 2 runs its K + 1 rows
    np.testing.assert_array_equal(window_items_host(LENGTHS, [(2, 3, 0)], K), [(2, 4), (2, 3)])
    np.testing.assert_array_equal(window_items_host(LENGTHS, [(4, 2, 0)], K), [(4, t) for t in range(2 + K, 1, -1)])
    # a dead sample alone: nothing, and no error
    for dead in ([(0, 0, 0)], [(-1, 0, 0)], [(6, 0, 0)], [(3, 12, 0)], [(3, -1, 0)]):
        assert window_items_host(LENGTHS, dead, K).shape == (0, 2)


@pytest.mark.parametrize("K", [1, 3, 10])
def test_random_batches(K):
    from mzgo.replay import window_items_host
    rng = np.random.default_rng(100 + K)
    for cap, B in ((1, 1), (7, 5), (300, 128), (64, 600)):
        length = rng.integers(0, 41, cap).astype(np.int32)
        length[rng.integers(0, cap, max(1, cap // 8))] = 0
        items = np.stack([rng.integers(-2, cap + 2, B), rng.integers(-2, 43, B), rng.integers(0, 8, B)], 1)
        got = window_items_host(length, items.astype(np.int32), K)
        np.testing.assert_array_equal(got, restated_items(length, items, K))


def test_twin_refusals():
    from mzgo._lib import MZGO_EINVAL, MZGO_OK, lib, ptr
    import ctypes
    length, items = np.array(LENGTHS, np.int32), np.array(ITEMS[:4], np.int32)
    out, n = np.zeros((4 * 64, 2), np.int32), ctypes.c_int32(-1)

    def call(length=length, cap=len(LENGTHS), items=items, B=4, K=3, out=out, n=ctypes.byref(n)):
        rc = lib.mzgo_replay_window_items_host(ptr(length), cap, ptr(items), B, K, ptr(out), n)
        return rc, lib.mzgo_last_error().decode()

    assert call()[0] == MZGO_OK and n.value == len(restated_items(LENGTHS, ITEMS[:4], 3))
    for kwargs, word in ((dict(length=None), "null length"), (dict(items=None), "null items"),
                         (dict(out=None), "null out"), (dict(n=None), "null n"), (dict(cap=0), "capacity"),
                         (dict(B=0), "B must be >= 1"), (dict(K=0), "unroll_steps 0"), (dict(K=64), "unroll_steps 64")):
        rc, msg = call(**kwargs)
        assert rc == MZGO_EINVAL and word in msg, (kwargs, rc, msg)
