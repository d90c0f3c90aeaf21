"""GPU checks of the arrival conv of the 9x9 LDS-tree search (sim_loop).

A select that reaches a lazily expanded node for the first time ends there,
and the node's parent conv always follows.  With MZGO_ARRIVAL_CONV on (read
at engine creation; the default) the conv starts at once: the node's policy
sums are formed at its head and wave 0 settles the node and picks under the
GEMM's second K half.  Only the order of independent steps changes, so
nothing may move: trees and self-play records are compared BYTE FOR BYTE with
the same run under MZGO_ARRIVAL_CONV=0, counters count for count, and the
new statistics (Engine.search_stats, mzgo_search_stats2) must show that the
path was taken, from both sources of the parent's Y.  9x9 / C = 96 only: the
path exists in no smaller build.  The switch's values 1 and 2 both mean "on":
the batch's picks under the conv, which 2 stood for, measured slower and are
not in the build.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_gpu_arrival import A, GAME, N, POSITIONS, SEED, _net, _obs, _state_dict
from test_gpu_value_cache import _same_bytes

pytestmark = pytest.mark.gpu

_OLD = ("batch_children_computed", "batch_children_cached", "batches_cut")
_NEW = ("arrival_convs_lds", "arrival_convs_l2")


class _Env:
    """Environment variables set for the making of one engine, then put back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_SEARCHES = {}


def _search(name, S, switch, cache=True, variant="self_play"):
    """One search of a position on a fresh engine -> (tree, root value bytes,
    stats, counters); each distinct search runs once per session."""
    key = (name, S, switch, cache, variant)
    if key not in _SEARCHES:
        from oracle.rng import injected_noise
        move = POSITIONS[name][0]
        with _Env(MZGO_ARRIVAL_CONV=str(switch), MZGO_VALUE_CACHE="1" if cache else "0"):
            eng = _net(_state_dict()).engine(num_games=1, num_simulations=S, seed=SEED, game_base=GAME,
                                             search_variant=variant)
        obs = torch.as_tensor(np.asarray(_obs(name)), dtype=torch.float32).reshape(1, 6, N, N)
        noise = torch.from_numpy(injected_noise(SEED, GAME, move, A))
        _, value = eng.search(obs, noise=noise, move_index=move)
        _SEARCHES[key] = (eng.tree(0), np.float64(value[0].item()).tobytes(), eng.search_stats(), eng.counters())
    return _SEARCHES[key]


@pytest.mark.parametrize("name,S", [(n, s) for n in ("late", "mid", "empty") for s in (64, 100)] + [("late", 200)])
def test_trees_identical_with_the_switch_at_0_1_2(name, S):
    t0, v0, s0, c0 = _search(name, S, 0)
    assert int(t0["visits"][0]) == S
    assert all(s0[k] == 0 for k in _NEW)
    for switch in (1, 2):
        t, v, s, c = _search(name, S, switch)
        print(f"{name} S={S} switch {switch}: {s} convs {c['dynamics_convs']} rows {c['prior_rows']}")
        _same_bytes(t, t0)
        assert v == v0
        assert {k: s[k] for k in _OLD} == {k: s0[k] for k in _OLD}
        assert (c["dynamics_convs"], c["prior_rows"]) == (c0["dynamics_convs"], c0["prior_rows"])


@pytest.mark.parametrize("S", range(60, 68))
def test_search_end_on_every_step_of_the_chain(S):
    """The late board's search ending at eight consecutive simulations: after
    an arrival with one simulation left (a single expansion behind the arrival
    conv), inside a batch that the end cuts short, and between them."""
    t0, v0, _, c0 = _search("late", S, 0)
    t2, v2, s2, c2 = _search("late", S, 2)
    print(f"late S={S}: {s2}")
    _same_bytes(t2, t0)
    assert v2 == v0
    assert (c2["dynamics_convs"], c2["prior_rows"]) == (c0["dynamics_convs"], c0["prior_rows"])


def test_both_sources_of_the_parents_y():
    """Late board, S = 200: with the value cache a cached batch leaves another
    node's Y in LDS, so some arrivals read their parent's Y from L2."""
    S = 200
    t_on, v_on, s_on, _ = _search("late", S, 2, cache=True)
    t_off, v_off, s_off, _ = _search("late", S, 2, cache=False)
    print(f"late S={S}: cache on {s_on} off {s_off}")
    _same_bytes(t_on, t_off)
    assert v_on == v_off
    _same_bytes(t_on, _search("late", S, 0, cache=True)[0])
    _same_bytes(t_off, _search("late", S, 0, cache=False)[0])
    assert s_on["arrival_convs_lds"] >= 1
    assert s_on["arrival_convs_l2"] >= 1


_EPOCHS = {}


def _epoch(switch, mode):
    """One self-play epoch of 4 games / 48 simulations on a fresh engine ->
    (packed records, counters, search statistics)."""
    key = (switch, mode)
    if key not in _EPOCHS:
        import mzgo
        from mzgo.distributed import pack_engine, slot_records, unpack
        with _Env(MZGO_ARRIVAL_CONV=str(switch), MZGO_MOVE_PARALLEL=mode, MZGO_QUEUE_HELPERS="0",
                  MZGO_TAIL_HELPERS="0"):
            sp = mzgo.SelfPlay(_net(_state_dict()), 4, 48, seed=1234)
            eng = sp.engine
            sp.reset(epoch=0)
            if mode == "1":
                sp.move(sp.max_moves)
            else:
                for _ in range(sp.max_moves):
                    sp.move()
            c = eng.counters()
        arrays = unpack(pack_engine(eng).cpu().numpy(), eng.G, eng.M, eng.N)
        # (record rows past a game's length are never written: compared up to
        # each game's length, as slot_records cuts them)
        recs = [slot_records(arrays, g) for g in range(eng.G)]
        whole = {k: arrays[k].copy() for k in ("meta", "status", "final")}
        _EPOCHS[key] = (recs, whole, c, eng.search_stats())
    return _EPOCHS[key]


@pytest.mark.parametrize("mode", ("1", "0"))
def test_selfplay_records_identical(mode):
    r0, w0, c0, s0 = _epoch(0, mode)
    r2, w2, c2, s2 = _epoch(2, mode)
    print(f"epoch mode={mode}: {s2} counters {c2}")
    for k in ("simulations", "moves", "games_finished", "dynamics_convs", "prior_rows"):
        assert c2[k] == c0[k], k
    assert c2["simulations"] == c2["moves"] * 48
    assert {k: s2[k] for k in _OLD} == {k: s0[k] for k in _OLD}
    for k in w0:
        np.testing.assert_array_equal(w2[k].view(np.uint8), w0[k].view(np.uint8), err_msg=k)
    for g, (a, b) in enumerate(zip(r2, r0)):
        assert a["length"] == b["length"] > 0 and a["status"] == b["status"]
        assert np.float64(a["final_reward"]).tobytes() == np.float64(b["final_reward"]).tobytes()
        for k in ("stones", "invd", "flags", "action", "value", "policy", "reward"):
            np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                          np.ascontiguousarray(b[k]).view(np.uint8), err_msg=f"slot {g} {k}")


@pytest.mark.parametrize("mode", ("1", "0"))
def test_the_switch_works(mode):
    _, _, _, s0 = _epoch(0, mode)
    _, _, c2, s2 = _epoch(2, mode)
    assert all(s0[k] == 0 for k in _NEW)
    n = s2["arrival_convs_lds"] + s2["arrival_convs_l2"]
    assert 0 < n <= c2["dynamics_convs"]


def test_old_stats_call_writes_three_values():
    from mzgo._lib import check, lib
    eng = _net(_state_dict()).engine(num_games=1, num_simulations=8)
    guard = 0xA5A5A5A5A5A5A5A5
    buf = np.full(4, guard, np.uint64)
    check(lib.mzgo_search_stats(eng._h, buf.ctypes.data_as(ctypes.c_void_p), None))
    assert int(buf[3]) == guard
    assert all(int(x) != guard for x in buf[:3])
    # the sized call writes min(cap, n) values and nothing past them
    for cap in (0, 2, 5, 8):
        buf = np.full(9, guard, np.uint64)
        check(lib.mzgo_search_stats2(eng._h, buf.ctypes.data_as(ctypes.c_void_p), cap, None))
        k = min(cap, 5)
        assert all(int(x) != guard for x in buf[:k]) and all(int(x) == guard for x in buf[k:])


def test_main_variant_keeps_its_tree():
    """main.py's select can end at a settled node without an action: it keeps
    the select-then-conv order whatever the switch says."""
    S = 64
    t0, v0, _, c0 = _search("mid", S, 0, variant="main")
    t2, v2, s2, c2 = _search("mid", S, 2, variant="main")
    print(f"main mid S={S}: {s2}")
    _same_bytes(t2, t0)
    assert v2 == v0
    assert (c2["dynamics_convs"], c2["prior_rows"]) == (c0["dynamics_convs"], c0["prior_rows"])
