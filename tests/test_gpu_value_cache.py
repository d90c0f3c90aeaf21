"""GPU checks of the value cache of the LDS trees' speculative batches (9x9).

When a batch at a leaf is cut short by its replay, the dropped children's
backup values are kept per (leaf, action); the leaf's next batch takes them
from there instead of expanding the children again.  A value depends on the
leaf's conv output and the action only, so nothing may move: the trees are
compared node for node with the oracle MCTS (tests/test_gpu_arrival.py's
positions, hooks and tolerances) and BYTE FOR BYTE with the same search
under MZGO_VALUE_CACHE=0 (read at engine creation), self-play records
likewise, and the search statistics (Engine.search_stats) must show that the
cache was used where re-batches exist and never across two searches of one
tree slot.
"""
import numpy as np
import pytest
import torch

from test_gpu_arrival import A, GAME, N, POSITIONS, SEED, _compare_trees, _net, _obs, _oracle_tree, _state_dict

pytestmark = pytest.mark.gpu

# Re-batches of the oracle's search of the late position (seed 31, game 2,
# move 160): maximal runs of consecutive simulations after the root phase with
# the same leaf, B >= 2, at a leaf that had such a run before -> (batches,
# children in them).  The device tree is the sequential one, so its cached
# children are these.
LATE_REBATCHES = {64: (9, 27), 100: (27, 79), 200: (75, 220)}

_TREE_KEYS = ("child", "visits", "value_sum", "prior", "root_prior")


def _search(name, S, cache, monkeypatch):
    """One search of a position on a fresh engine -> (tree, root value, stats, engine)."""
    from oracle.rng import injected_noise
    monkeypatch.setenv("MZGO_VALUE_CACHE", "1" if cache else "0")
    move = POSITIONS[name][0]
    eng = _net(_state_dict()).engine(num_games=1, num_simulations=S, seed=SEED, game_base=GAME)
    obs = torch.as_tensor(np.asarray(_obs(name)), dtype=torch.float32).reshape(1, 6, N, N)
    noise = torch.from_numpy(injected_noise(SEED, GAME, move, A))
    _, value = eng.search(obs, noise=noise, move_index=move)
    return eng.tree(0), float(value[0].item()), eng.search_stats(), eng


def _same_bytes(ta, tb):
    """Two exported trees, byte for byte.  (Row 0 of ``prior`` is left out: the
    root's priors are ``root_prior``, the row is never written and holds what
    its allocation held -- the two trees come from two engines.)"""
    assert int(ta["n"]) == int(tb["n"])
    for k in _TREE_KEYS:
        xa, xb = (ta[k][1:], tb[k][1:]) if k == "prior" else (ta[k], tb[k])
        np.testing.assert_array_equal(np.ascontiguousarray(xa).view(np.uint8),
                                      np.ascontiguousarray(xb).view(np.uint8), err_msg=k)


@pytest.mark.parametrize("S", (64, 100, 200))
def test_late_position_cache_on_equals_off_and_oracle(S, monkeypatch):
    move = POSITIONS["late"][0]
    r_root, r_value, r_actions = _oracle_tree("late", S, move)
    t_on, v_on, s_on, _ = _search("late", S, True, monkeypatch)
    t_off, v_off, s_off, _ = _search("late", S, False, monkeypatch)
    print(f"late S={S}: on {s_on} off {s_off}")
    assert int(t_on["visits"][0]) == S
    assert abs(v_on - r_value) < 1e-5
    _compare_trees(t_on, r_root, r_actions, A)
    _same_bytes(t_on, t_off)
    assert np.float64(v_on).tobytes() == np.float64(v_off).tobytes()
    assert s_off["batch_children_cached"] == 0
    assert s_on["batch_children_cached"] > 0
    assert s_on["batch_children_computed"] + s_on["batch_children_cached"] == s_off["batch_children_computed"]
    assert s_on["batches_cut"] == s_off["batches_cut"] > 0
    assert s_on["batch_children_cached"] == LATE_REBATCHES[S][1]


def test_mid_position_has_no_cut_and_no_cached_child(monkeypatch):
    S = 64
    move = POSITIONS["mid"][0]
    r_root, r_value, r_actions = _oracle_tree("mid", S, move)
    t_on, v_on, s_on, _ = _search("mid", S, True, monkeypatch)
    t_off, v_off, s_off, _ = _search("mid", S, False, monkeypatch)
    print(f"mid S={S}: on {s_on} off {s_off}")
    assert s_on["batch_children_cached"] == 0 and s_on["batches_cut"] == 0
    assert s_on == s_off
    assert abs(v_on - r_value) < 1e-5
    _compare_trees(t_on, r_root, r_actions, A)
    _same_bytes(t_on, t_off)


def _epoch(cache, mode, S, monkeypatch):
    """One self-play epoch of 4 games on a fresh engine -> (per-slot records,
    whole-engine fields, counters, search statistics)."""
    import mzgo
    from mzgo.distributed import pack_engine, slot_records, unpack
    monkeypatch.setenv("MZGO_VALUE_CACHE", "1" if cache else "0")
    monkeypatch.setenv("MZGO_MOVE_PARALLEL", mode)
    monkeypatch.setenv("MZGO_QUEUE_HELPERS", "0")
    monkeypatch.setenv("MZGO_TAIL_HELPERS", "0")
    sp = mzgo.SelfPlay(_net(_state_dict()), 4, S, seed=1234)
    eng = sp.engine
    sp.reset(epoch=0)
    if mode == "1":
        sp.move(sp.max_moves)
    else:
        for _ in range(sp.max_moves):
            sp.move()
    c = eng.counters()
    arrays = unpack(pack_engine(eng).cpu().numpy(), eng.G, eng.M, eng.N)
    # (the two runs are two engines: record rows past a game's length are never
    # written and hold whatever their allocation held, so the records are
    # compared up to each game's length, as slot_records cuts them)
    recs = [slot_records(arrays, g) for g in range(eng.G)]
    whole = {k: arrays[k].copy() for k in ("meta", "status", "final")}
    return recs, whole, {k: c[k] for k in ("simulations", "moves", "dynamics_convs", "prior_rows")}, eng.search_stats()


@pytest.mark.parametrize("mode", ("1", "0"))
def test_selfplay_epoch_cache_on_equals_off(mode, monkeypatch):
    """9x9 / 4 games / 100 simulations: the move-parallel epoch (the search
    queue) and one launch per move (k_selfplay_move), each against the same
    run without the cache.  (At S = 48 this epoch has one cut batch and no
    re-batch: nothing would be taken from the cache; at 100 it has 55 cuts and
    41 cached children.)"""
    S = 100
    r_on, w_on, c_on, s_on = _epoch(True, mode, S, monkeypatch)
    print(f"epoch mode={mode} S={S}: on {s_on} counters {c_on}")
    r_off, w_off, c_off, s_off = _epoch(False, mode, S, monkeypatch)
    print(f"epoch mode={mode} S={S}: off {s_off}")
    assert c_on == c_off, (c_on, c_off)
    assert c_on["simulations"] == c_on["moves"] * S
    for k in w_on:
        np.testing.assert_array_equal(w_on[k].view(np.uint8), w_off[k].view(np.uint8), err_msg=k)
    for g, (a, b) in enumerate(zip(r_on, r_off)):
        assert a["length"] == b["length"] > 0 and a["status"] == b["status"]
        assert np.float64(a["final_reward"]).tobytes() == np.float64(b["final_reward"]).tobytes()
        for k in ("stones", "invd", "flags", "action", "value", "policy", "reward"):
            np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                          np.ascontiguousarray(b[k]).view(np.uint8), err_msg=f"slot {g} {k}")
    assert s_off["batch_children_cached"] == 0
    assert s_on["batch_children_cached"] > 0
    assert s_on["batch_children_computed"] + s_on["batch_children_cached"] == s_off["batch_children_computed"]
    assert s_on["batches_cut"] == s_off["batches_cut"]


def test_second_search_in_a_slot_starts_with_an_empty_cache(monkeypatch):
    """The late position, then the mid-game one, in the same tree slot: the
    second search takes nothing from the cache and equals a fresh engine's."""
    from oracle.rng import injected_noise
    S = 64
    _, _, s1, eng = _search("late", S, True, monkeypatch)
    assert s1["batch_children_cached"] > 0
    move = POSITIONS["mid"][0]
    obs = torch.as_tensor(np.asarray(_obs("mid")), dtype=torch.float32).reshape(1, 6, N, N)
    eng.search(obs, noise=torch.from_numpy(injected_noise(SEED, GAME, move, A)), move_index=move)
    t2, s2 = eng.tree(0), eng.search_stats()
    assert s2["batch_children_cached"] == s1["batch_children_cached"]
    assert s2["batches_cut"] == s1["batches_cut"]
    t_fresh, _, _, _ = _search("mid", S, True, monkeypatch)
    _same_bytes(t2, t_fresh)


def test_main_variant_late_position_matches_oracle(monkeypatch):
    """search_variant="main" takes the same path under the other select."""
    import mzgo
    from oracle.mcts import tree_summary
    from oracle.mcts_main import MCTSMain
    from oracle.net import OracleNet
    from oracle.rng import SearchHooks, injected_noise
    monkeypatch.setenv("MZGO_VALUE_CACHE", "1")
    S, seed, game = 100, 17, 1
    moves = POSITIONS["late"][0]
    obs = _obs("late")
    noise = injected_noise(seed, game, moves, A)
    hooks = SearchHooks(seed, game, moves)
    sd = _state_dict()
    ref = MCTSMain(OracleNet(sd), A, S, choice=lambda seq, sim: seq[hooks.choice_index(len(seq), sim)],
                   noise=lambda p, a, e: (1 - e) * p + e * noise)
    with torch.no_grad():
        r_root = ref.run(obs)
    net = _net(sd)
    m = mzgo.MainMCTS(net, A, S, seed=seed, game=game)
    root = m.run(obs, move_index=moves, noise=torch.from_numpy(noise))
    stats = net.engine(num_games=1, num_simulations=S, **m._m.cfg).search_stats()
    print(f"main late S={S}: {stats}")
    assert stats["batch_children_cached"] > 0
    np.testing.assert_array_equal(tree_summary(root, A)[0], tree_summary(r_root, A)[0])
    np.testing.assert_array_equal(np.array(tree_summary(root, A)[1]), np.array(tree_summary(r_root, A)[1]))
    assert abs(m.root_value - r_root.value()) < 1e-5
