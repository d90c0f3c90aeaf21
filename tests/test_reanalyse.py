"""CPU: the host side of reanalysis (mzgo.reanalyse) -- the record format of
positions, the search keys of self-play records, argument checks."""
import numpy as np
import pytest
import torch


def _random_records(N, n, seed):
    rng = np.random.default_rng(seed)
    stones = rng.integers(0, 3, size=(n, N * N)).astype(np.int8)
    invd = ((stones > 0) | (rng.random((n, N * N)) < 0.1)).astype(np.uint8)
    flags = (np.arange(n) % 8).astype(np.uint8)            # every (turn, passed, done) combination
    return stones, invd, flags


@pytest.mark.parametrize("N", [5, 9, 19])
def test_positions_from_planes_inverts_planes(N):
    from mzgo.reanalyse import positions_from_planes
    from mzgo.trainer import _planes
    stones, invd, flags = _random_records(N, 16, N)
    obs = np.stack([_planes(stones[i], invd[i], int(flags[i]), N) for i in range(len(flags))])
    for inp in (obs, torch.from_numpy(obs), torch.from_numpy(obs).float(), list(obs)):
        s, i, f = positions_from_planes(inp)
        assert (s.dtype, i.dtype, f.dtype) == (torch.int8, torch.uint8, torch.uint8)
        np.testing.assert_array_equal(s.numpy(), stones)
        np.testing.assert_array_equal(i.numpy(), invd)
        np.testing.assert_array_equal(f.numpy(), flags)
    # ... and back
    s, i, f = positions_from_planes(obs)
    again = np.stack([_planes(s[k].numpy(), i[k].numpy(), int(f[k]), N) for k in range(len(f))])
    np.testing.assert_array_equal(again, obs)
    with pytest.raises(ValueError):
        positions_from_planes(obs[:, :5])


def test_observation_planes_and_positions_from_planes_invert_each_other():
    """One random 5x5 position under every combination of the three flag bits:
    record -> observation -> record and observation -> record -> observation
    are the identity, and each plane is what the record says."""
    from mzgo.reanalyse import observation_planes, positions_from_planes
    from mzgo.trainer import _planes
    assert _planes is observation_planes                        # the one Python plane builder
    N = 5
    rng = np.random.default_rng(50)
    stones = rng.integers(0, 3, size=N * N).astype(np.int8)
    invd = rng.integers(0, 2, size=N * N).astype(np.uint8)
    assert set(stones) == {0, 1, 2} and set(invd) == {0, 1}
    for flags in range(8):
        obs = observation_planes(stones, invd, flags, N)
        assert obs.dtype == np.float64 and obs.shape == (6, N, N)
        np.testing.assert_array_equal(obs[0].reshape(-1), stones == 1)
        np.testing.assert_array_equal(obs[1].reshape(-1), stones == 2)
        np.testing.assert_array_equal(obs[3].reshape(-1), invd)
        for plane, bit in ((2, 0), (4, 1), (5, 2)):
            np.testing.assert_array_equal(obs[plane], np.full((N, N), (flags >> bit) & 1))
        s, i, f = positions_from_planes(obs[None])
        np.testing.assert_array_equal(s[0].numpy(), stones)
        np.testing.assert_array_equal(i[0].numpy(), invd)
        assert int(f[0]) == flags
        np.testing.assert_array_equal(observation_planes(s[0].numpy(), i[0].numpy(), f[0], N), obs)
        # bit 3 (the fast-search bit of a stored row's flags) shows in no plane
        np.testing.assert_array_equal(observation_planes(stones, invd, np.uint8(flags | 8), N), obs)


def _move_key_id(game_base, g, epoch):
    """csrc/mzgo_move.hpp move_key: (uint32_t)(game_base + g) ^ ((uint32_t)epoch << 24), as the int32 the ABI takes."""
    u = ((game_base + g) & 0xFFFFFFFF) ^ ((epoch << 24) & 0xFFFFFFFF)
    return u - (1 << 32) if u >= 1 << 31 else u


def test_record_ids_match_move_key():
    from mzgo.reanalyse import record_ids
    for game_base, g, epoch in [(0, 0, 0), (0, 3, 1), (1000, 255, 2), (5, 7, 127), (5, 7, 128), (5, 7, 255),
                                (1 << 24, 1, 1), (70000, 12, 300)]:
        ids = record_ids(game_base, g, epoch, np.arange(4))
        assert ids.dtype == np.int32 and ids.shape == (4, 2)
        assert ids[:, 0].tolist() == [_move_key_id(game_base, g, epoch)] * 4
        assert ids[:, 1].tolist() == [0, 1, 2, 3]
    ids = record_ids(10, np.array([0, 1, 2]), 1, np.array([5, 6, 7]))
    assert ids.tolist() == [[_move_key_id(10, k, 1), 5 + k] for k in range(3)]
    assert record_ids(0, 2, 0, 9).tolist() == [[2, 9]]


def test_latest_first_is_a_stable_sort_by_falling_move():
    from mzgo.reanalyse import latest_first, record_ids
    ids = np.concatenate([record_ids(0, g, 0, np.arange(L)) for g, L in enumerate([3, 1, 4])])
    order = latest_first(ids)
    assert sorted(order.tolist()) == list(range(8))
    assert ids[order].tolist() == [[2, 3], [0, 2], [2, 2], [0, 1], [2, 1], [0, 0], [1, 0], [2, 0]]


def test_reanalyser_rejects_other_board_size():
    import mzgo
    from mzgo.reanalyse import Reanalyser
    net = mzgo.MuZeroNet(96, 5 * 5 + 1)
    ra = Reanalyser(net, 8, slots=2)
    traj = {"observations": [np.zeros((6, 9, 9))] * 4, "actions": [0, 1], "rewards": [0.0, 0.0, 0.0],
            "policies": [np.full(82, 1 / 82)] * 2}
    with pytest.raises(ValueError, match="9"):
        ra.run([traj])
    good = {"observations": [np.zeros((6, 5, 5))] * 4, "actions": [0, 1], "rewards": [0.0, 0.0, 0.0],
            "policies": [np.full(26, 1 / 26)] * 2}
    with pytest.raises(ValueError, match="ids"):
        ra.run([good], ids=[np.zeros((3, 2), np.int32)])
