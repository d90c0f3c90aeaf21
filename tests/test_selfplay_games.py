"""CPU checks of continuous self-play (mzgo_replay_play_games): the queue's
identity rule on the host, the entry point's null-handle refusals (no device
call is made), and the seed tests/test_gpu_selfplay_games.py's compat
"reference" case relies on."""
import numpy as np
import pytest


@pytest.mark.parametrize("n,G,game_base,epoch", [(1, 1, 0, 0), (12, 4, 0, 0), (10, 4, 7, 3), (7, 3, 5, 0),
                                                 (5, 8, 1000, 2), (600, 256, 256, 126), (9, 2, 0, 255)])
def test_queue_key_gids_are_slot_and_epoch_record_ids(n, G, game_base, epoch):
    from mzgo.reanalyse import record_ids
    from mzgo.replay import queue_key_gids
    got = queue_key_gids(n, G, game_base, epoch)
    assert got.dtype == np.int32 and got.shape == (n,)
    for j in range(n):
        assert got[j] == record_ids(game_base, j % G, epoch + j // G, [0])[0, 0], j
    assert len(set(got.tolist())) == n           # no two games of a call share a key


def test_queue_key_gids_is_public():
    import mzgo
    from mzgo.replay import queue_key_gids
    assert mzgo.queue_key_gids is queue_key_gids and "queue_key_gids" in mzgo.__all__
    assert queue_key_gids(0, 4).shape == (0,)


def test_null_handles_are_refused_with_a_message():
    from mzgo._lib import MZGO_EINVAL, lib
    assert lib.mzgo_replay_play_games(None, None, 1, 0, None) == MZGO_EINVAL
    msg = lib.mzgo_last_error().decode()
    assert "mzgo_replay_play_games" in msg and "null replay" in msg


def test_symbol_is_exported_and_bound():
    import re
    import subprocess

    from mzgo import _lib
    assert "mzgo_replay_play_games" in _lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT mzgo_replay_play_games\b", out)


def _reference_compat_game(seed, kid, N, max_moves, temperature_moves=15, pass_epsilon=0.01):
    """(moves, ended by double pass) of a compat "reference" game with key id
    ``kid``: the move is a draw over the legal actions
    -- np.random.choice's inverse CDF on mask / sum while the temperature is
    on, random.choice afterwards -- so the boards need no network."""
    from oracle import gogame, rng
    from oracle.mcts import root_valid_mask
    from oracle.selfplay import inverse_cdf
    state, mv = gogame.init_state(N), 0
    while not gogame.game_ended(state) and mv < max_moves:
        mask = root_valid_mask(state, pass_epsilon)
        h = rng.draw(rng.stream_key(seed, int(kid), mv), rng.TAG_ACTION, 0)
        if mv < temperature_moves:
            action = inverse_cdf(mask / mask.sum(), rng.u01(h))
        else:
            legal = np.where(mask > 0)[0]
            action = int(legal[rng.randbelow(h, len(legal))])
        state = gogame.next_state(state, action)
        mv += 1
    return mv, bool(gogame.game_ended(state))


def test_the_reference_compat_seed_ends_games_both_ways():
    """test_reference_compat_games_end_both_ways' shape (5x5, G = 4, n = 12,
    max_moves 60, seed 2): games at the move cap and games ended by double
    pass, so the ingest's -0.5 rule and its winner rule are both crossed."""
    from mzgo.replay import queue_key_gids
    ends = [_reference_compat_game(2, int(kid) & 0xFFFFFFFF, 5, 60) for kid in queue_key_gids(12, 4, 0, 0)]
    capped = [j for j, (L, done) in enumerate(ends) if L == 60 and not done]
    passed = [j for j, (L, done) in enumerate(ends) if done]
    assert capped == [4, 8] and len(passed) == 10
