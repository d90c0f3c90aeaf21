"""The move-parallel epoch's boards launch (k_selfplay_boards) against the CPU
oracle.

The launch keeps a game's board and its groups (labels, liberties) in LDS
from move to move, updates the groups per move instead of labelling the board
from scratch, stores the slot's board once when the game's loop ends and adds
its counters once per game.  Whole games are therefore replayed on
oracle/gogame.py: every move's recorded board, INVD plane, flags, action and
reward, each game's length, status, final reward and final board -- on games
that contain the cases the incremental groups can get wrong (a capture of
several stones, a ko, a double pass; found on the CPU, by the oracle, before
anything runs on the GPU).

Under compat "reference" the action never reads the search (SURVEY.md section
0.6: the visit counts select_action sees are zeros), so the oracle's
select_action is run with a search stub that returns those zeros: the action
rule and the counter streams are the oracle's own code.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gogame as gg
from oracle import selfplay as osp
from oracle.rng import SearchHooks

pytestmark = pytest.mark.gpu

S = 2                     # simulations per move: the boards never read the searches
TEMPERATURE_MOVES = 15    # SelfPlay's default


class _NoSearch:
    """MCTS stand-in: compat "reference" hands select_action zero visit counts."""

    def __init__(self, net, action_size, num_simulations, **kw):
        self.A = action_size

    def run(self, observation):
        return None, np.zeros(self.A), 0.0


def _oracle_game(N, seed, gid, temperature_moves):
    """One game by the oracle alone: states before each move, actions, rewards,
    the final state, and what happened on the way."""
    A, M = N * N + 1, N * N
    agent = osp.Agent(None, N, A, S, compat="reference")
    st = gg.init_state(N)
    states, actions, rewards = [], [], []
    big_capture = ko = False
    for mv in range(M):
        t = 1.0 if mv < temperature_moves else 0
        a, _, _ = agent.select_action(st, t, SearchHooks(seed, gid, mv))
        states.append(st)
        actions.append(a)
        player = int(gg.turn(st))
        nxt = gg.next_state(st, a)
        lost = int(st[1 - player].sum() - nxt[1 - player].sum())
        big_capture |= lost > 1
        # a ko point is the one INVD entry the suicide rule alone does not give
        plain = gg.compute_invalid_moves(nxt, player)
        ko |= bool((nxt[gg.INVD_CHNL] != plain).any())
        st = nxt
        ended = bool(gg.game_ended(st))
        rewards.append(float(gg.winning(st)) if ended else 0.0)
        if ended:
            break
    ended = bool(gg.game_ended(st))
    return dict(states=states, actions=actions, rewards=rewards, final=st, ended=ended,
                final_reward=float(gg.winning(st)) if ended else 0.0, big_capture=big_capture, ko=ko)


@functools.lru_cache(maxsize=None)
def _oracle_games(N, G, temperature_moves, need_cases):
    """The oracle's games of the first seed whose games hold every case (5x5),
    computed once and shared by the tests."""
    real = osp.MCTS
    osp.MCTS = _NoSearch
    try:
        for seed in range(1000, 1040):
            games = [_oracle_game(N, seed, g, temperature_moves) for g in range(G)]
            if not need_cases or (any(x["big_capture"] for x in games) and any(x["ko"] for x in games)
                                  and any(x["ended"] for x in games)):
                return seed, games
    finally:
        osp.MCTS = real
    raise AssertionError("no seed with a multi-stone capture, a ko and a double pass")


def _net(N, C=96):
    import mzgo
    from oracle.weights import deterministic_state_dict
    net = mzgo.MuZeroNet(C, N * N + 1).to("cuda").eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state_dict(C, N * N + 1, 0).items()})
    return net


def _arrays(eng):
    from mzgo.distributed import pack_engine, unpack
    return unpack(pack_engine(eng).cpu().numpy(), eng.G, eng.M, eng.N)


def _planes(st):
    """(stones, invd, flags) of a GymGo state, as the engine records them."""
    stones = (st[0] > 0).astype(np.int8) + 2 * (st[1] > 0).astype(np.int8)
    flags = int(st[2].max()) | (int(st[4].max() == 1) << 1) | (int(st[5].max() == 1) << 2)
    return stones.reshape(-1), (st[3] > 0).astype(np.uint8).reshape(-1), flags


def _check_against_oracle(sp, arrays, games, N):
    from mzgo.distributed import slot_records
    planes = sp.engine.board_planes().cpu().numpy()
    for g, o in enumerate(games):
        r = slot_records(arrays, g)
        L = len(o["actions"])
        assert r["length"] == L, (g, r["length"], L)
        assert r["status"] == 1, (g, r["status"])
        np.testing.assert_array_equal(r["action"], np.array(o["actions"]), err_msg=f"game {g} actions")
        np.testing.assert_array_equal(r["reward"], np.array(o["rewards"]), err_msg=f"game {g} rewards")
        for mv, st in enumerate(o["states"]):
            stones, invd, flags = _planes(st)
            np.testing.assert_array_equal(r["stones"][mv], stones, err_msg=f"game {g} move {mv} stones")
            np.testing.assert_array_equal(r["invd"][mv], invd, err_msg=f"game {g} move {mv} invd")
            assert int(r["flags"][mv]) & 7 == flags, (g, mv, int(r["flags"][mv]), flags)
        assert r["final_reward"] == o["final_reward"], (g, r["final_reward"], o["final_reward"])
        np.testing.assert_array_equal(planes[g], o["final"], err_msg=f"game {g} final board")


@pytest.mark.parametrize("N,G", [(5, 64), (9, 16)], ids=["5x5_g64", "9x9_g16"])
def test_boards_launch_matches_oracle_games(N, G):
    import mzgo
    seed, games = _oracle_games(N, G, TEMPERATURE_MOVES, N == 5)
    if N == 5:
        assert any(x["big_capture"] for x in games) and any(x["ko"] for x in games)
        assert any(x["ended"] for x in games)                  # a double pass
    sp = mzgo.SelfPlay(_net(N), G, S, seed=seed)
    sp.reset(epoch=0)
    sp.move(sp.max_moves)
    c = sp.engine.counters()
    assert c["playing"] == 0
    _check_against_oracle(sp, _arrays(sp.engine), games, N)


@pytest.mark.parametrize("temperature_moves", [25, 0], ids=["all_moves_sampled", "no_move_sampled"])
def test_temperature_schedule_matches_oracle_select_action(temperature_moves):
    """The inverse CDF (every move) and the uniform pick (no move)."""
    import mzgo
    N, G = 5, 64
    seed, games = _oracle_games(N, G, temperature_moves, False)
    sp = mzgo.SelfPlay(_net(N), G, S, seed=seed, temperature_moves=temperature_moves)
    sp.reset(epoch=0)
    sp.move(sp.max_moves)
    _check_against_oracle(sp, _arrays(sp.engine), games, N)


def _run(sp, chunks, epoch):
    eng = sp.engine
    c0 = eng.counters()
    sp.reset(epoch=epoch)
    for k in chunks:
        sp.move(k)
    c1 = eng.counters()
    return _arrays(eng), eng.board_planes().cpu().numpy(), \
        {k: c1[k] - c0[k] for k in ("moves", "simulations", "games_finished")}


def test_counters_equal_the_game_per_workgroup_launch(monkeypatch):
    import mzgo
    N, G = 5, 64
    sp = mzgo.SelfPlay(_net(N), G, S, seed=1000)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MZGO_MOVE_PARALLEL", mode)
        out[mode] = _run(sp, [sp.max_moves], 1)
    assert out["1"][2] == out["0"][2], (out["1"][2], out["0"][2])
    assert out["1"][2]["games_finished"] == G
    assert out["1"][2]["moves"] == int(out["1"][0]["meta"][:, 3].sum())
    assert out["1"][2]["simulations"] == S * out["1"][2]["moves"]


@pytest.mark.parametrize("N,G,chunks", [(5, 64, [4, 3, 18]), (9, 16, [5, 1, 75])], ids=["5x5", "9x9"])
def test_launches_that_start_mid_game_equal_one_launch(N, G, chunks):
    """A launch that finds stones on the board labels its groups from scratch
    once and goes on incrementally: the same records, boards and counters as
    the whole game in one launch."""
    import mzgo
    sp = mzgo.SelfPlay(_net(N), G, S, seed=1001)
    assert sum(chunks) == sp.max_moves
    one, planes_one, c_one = _run(sp, [sp.max_moves], 2)
    many, planes_many, c_many = _run(sp, chunks, 2)
    assert c_one == c_many, (c_one, c_many)
    for k in one:
        np.testing.assert_array_equal(one[k].view(np.uint8), many[k].view(np.uint8), err_msg=k)
    np.testing.assert_array_equal(planes_one, planes_many)
