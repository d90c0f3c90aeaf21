"""Playout cap randomization on the GPU: self-play moves searched with the
full budget S with probability p and the fast budget F otherwise, the record
flag (bit 3), the store's policy mask and reanalysis' unmasking.

The budget of a move is ``mzgo.playout_budget_host(seed, key_gid, move, S, F,
p)`` -- the host twin of the function the three self-play schedules run -- so
every expectation here is formed on the host from the key alone.  The seeds
are tests/test_playout_cap.py's (``GPU_CASES``), which asserts that each game
has at least 5 fast and 5 full moves among its first 12.
"""
import numpy as np
import pytest
import torch

from test_playout_cap import GPU_CASES, GPU_P, budgets

pytestmark = pytest.mark.gpu

FAST = 8                                   # record flags bit 3
FIELDS = ("stones", "invd", "action", "value", "policy", "reward")
# main.py's search on a SelfPlay engine (tests/test_gpu_reanalyse.py's MAIN)
MAIN = dict(c_puct=2.0, dirichlet_alpha=0.03, dirichlet_epsilon=0.25, pass_epsilon=0.05, search_variant="main")
# (case, search variant): both variants at 5x5 and 9x9, and MainSelfPlay's own 6x6 C = 128 shape
VARIANT_CASES = [("5x5", "self_play"), ("5x5", "main"), ("9x9", "self_play"), ("9x9", "main"), ("6x6main", "main")]


def _net(N, C=96, seed=0):
    import mzgo
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A).cuda().eval()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, seed))
    return net


def _case(name):
    N, G, S, F, seed, _ = GPU_CASES[name]
    return N, G, S, F, seed


def _selfplay(name, net=None, *, S=None, caps=True, p=GPU_P, compat="fixed", variant="self_play", **kw):
    """The case's SelfPlay under ``variant``'s search: with the caps, or plain with S simulations."""
    import mzgo
    N, G, S0, F, seed = _case(name)
    if variant == "main":
        kw = {**MAIN, **kw}
    if N == 19:
        kw.setdefault("max_moves", 12)
    cap = dict(fast_simulations=F, full_search_prob=p) if caps else {}
    return mzgo.SelfPlay(net or _net(N), G, S or S0, seed=seed, compat=compat, **cap, **kw)


def _main_selfplay(net=None, *, S=None, caps=True, p=GPU_P):
    from mzgo.trainer import MainSelfPlay
    N, G, S0, F, seed = _case("6x6main")
    cap = dict(fast_simulations=F, full_search_prob=p) if caps else {}
    return MainSelfPlay(net or _net(N, 128, 5), G, S or S0, seed=seed, **cap)


def _play(sp, per_move=False, epoch=0):
    """Whole games in the slots; returns (records, counter deltas)."""
    eng = sp.engine
    c0 = eng.counters()
    sp.reset(epoch)
    if per_move:
        for _ in range(sp.max_moves):
            sp.move()
    else:
        sp.move(sp.max_moves)
    c1 = eng.counters()
    assert c1["playing"] == 0
    return [eng.record(g) for g in range(sp.G)], {k: c1[k] - c0[k] for k in ("simulations", "moves", "games_finished")}


def _same_records(a, b, flag_mask=0xFF):
    """tests/test_gpu_reanalyse.py's comparison; the flags under ``flag_mask``."""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra["length"] == rb["length"] and ra["status"] == rb["status"]
        assert ra["final_reward"] == rb["final_reward"]
        for k in FIELDS:
            assert ra[k].tobytes() == rb[k].tobytes(), k
        assert (ra["flags"] & flag_mask).tobytes() == (rb["flags"] & flag_mask).tobytes(), "flags"


def _host_budgets(sp, g, L, S, F, p=GPU_P, epoch=0):
    from mzgo.reanalyse import record_ids
    kid = int(record_ids(sp.game_base, g, epoch, [0])[0, 0]) & 0xFFFFFFFF
    return budgets(sp._engine_args["seed"], kid, L, S, F, p)


def _check_flags(sp, recs, S, F, p=GPU_P, epoch=0):
    """Bit 3 of every record row is the host twin's budget; returns (fast rows, full rows, the budgets' sum)."""
    n_fast = n_full = total = 0
    for g, r in enumerate(recs):
        want = _host_budgets(sp, g, r["length"], S, F, p, epoch)
        got = [F if f & FAST else S for f in r["flags"]]
        assert got == want, (g, got, want)
        n_fast += want.count(F)
        n_full += want.count(S)
        total += sum(want)
    return n_fast, n_full, total


# ---------------------------------------------------------------------------
# 1. off is the parent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("name", ["5x5", "9x9"])
def test_full_search_prob_one_is_an_engine_without_caps(name, compat):
    N, G, S, F, seed = _case(name)
    net = _net(N)
    capped = _selfplay(name, net, p=1.0, compat=compat)
    plain = _selfplay(name, net, caps=False, compat=compat)
    assert capped.engine is not plain.engine and capped.engine.config.fast_simulations == F
    (ra, ca), (rb, cb) = _play(capped), _play(plain)
    _same_records(ra, rb)
    assert not any((r["flags"] & FAST).any() for r in ra)
    assert ca == cb and ca["simulations"] == ca["moves"] * S


# ---------------------------------------------------------------------------
# 2. all fast is a smaller engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", VARIANT_CASES)
def test_all_fast_is_an_engine_with_the_fast_budget(name, variant):
    N, G, S, F, seed = _case(name)
    if name == "6x6main":
        net = _net(N, 128, 5)
        capped, small = _main_selfplay(net, p=0.0).sp, _main_selfplay(net, S=F, caps=False).sp
    else:
        net = _net(N)
        capped = _selfplay(name, net, p=0.0, variant=variant)
        small = _selfplay(name, net, S=F, caps=False, variant=variant)
        assert capped.engine.config.search_variant == variant
    (ra, ca), (rb, cb) = _play(capped), _play(small)
    _same_records(ra, rb, flag_mask=0xFF ^ FAST)
    for r, q in zip(ra, rb):
        assert r["length"] > 0 and (r["flags"] & FAST).all() and not (q["flags"] & FAST).any()
    assert ca == cb and ca["simulations"] == ca["moves"] * F


# ---------------------------------------------------------------------------
# 3. each move is the search its flag names
# ---------------------------------------------------------------------------
def _reanalysed(eng, sp, recs):
    """Every recorded position through ``eng``'s reanalysis queue under the record's own key:
    per game (value bits [L], policy bits [L, A])."""
    from mzgo.reanalyse import record_ids
    lens = [r["length"] for r in recs]
    ids = np.concatenate([record_ids(sp.game_base, g, 0, np.arange(L)) for g, L in enumerate(lens)])
    _, value, policy = eng.reanalyse(np.concatenate([r["stones"] for r in recs]),
                                     np.concatenate([r["invd"] for r in recs]),
                                     np.concatenate([r["flags"] for r in recs]), ids)      # (bit 3 included: ignored)
    value, policy = value.cpu().numpy(), policy.cpu().numpy()
    out, at = [], 0
    for L in lens:
        out.append((value[at:at + L].view(np.uint64), policy[at:at + L].view(np.uint64)))
        at += L
    return out


@pytest.mark.parametrize("name,variant", VARIANT_CASES + [("19x19", "self_play")])
def test_each_move_is_the_search_its_flag_names(name, variant):
    N, G, S, F, seed = _case(name)
    if name == "6x6main":
        net = _net(N, 128, 5)
        sp = _main_selfplay(net).sp
    else:
        net = _net(N)
        sp = _selfplay(name, net, variant=variant)
    recs, c = _play(sp)
    n_fast, n_full, total = _check_flags(sp, recs, S, F)
    assert n_fast > 0 and n_full > 0
    assert c["simulations"] == total and c["moves"] == n_fast + n_full
    # two plain engines, the same weights, seed and options, one per budget
    args = dict(sp._engine_args)
    args.pop("fast_simulations"), args.pop("full_search_prob")
    by_budget = {b: _reanalysed(net.engine(G, b, **args), sp, recs) for b in (S, F)}
    for g, r in enumerate(recs):
        for t in range(r["length"]):
            mine, other = (F, S) if r["flags"][t] & FAST else (S, F)
            v, pol = by_budget[mine][g]
            assert r["value"][t:t + 1].view(np.uint64)[0] == v[t], (g, t)
            assert r["policy"][t].view(np.uint64).tobytes() == pol[t].tobytes(), (g, t)
    # the caps are self-play's alone: reanalysis and Engine.search on the capped engine itself are the S engine's
    own = _reanalysed(sp.engine, sp, recs)
    for g in range(G):
        assert np.array_equal(own[g][0], by_budget[S][g][0]) and np.array_equal(own[g][1], by_budget[S][g][1]), g
    obs = torch.zeros(G, 6, N, N)
    for mv in range(4):                        # (moves whose self-play budgets differ)
        (va, wa), (vb, wb) = sp.engine.search(obs, move_index=mv), net.engine(G, S, **args).search(obs, move_index=mv)
        assert torch.equal(va, vb) and torch.equal(wa.view(torch.int64), wb.view(torch.int64)), mv
        assert int(va.sum()) > F * G
    # (the two budgets are different searches: the comparison above can tell them apart)
    assert any(not np.array_equal(by_budget[S][g][1], by_budget[F][g][1]) for g in range(G))


def test_the_arena_ignores_the_caps():
    """An engine whose every self-play move would be fast (p = 0) plays arena games as the engine without caps."""
    N, G, S, F, seed = _case("5x5")
    net, opp = _net(N), _net(N, seed=1)
    out = []
    for caps in (True, False):
        sp = _selfplay("5x5", net, caps=caps, p=0.0, variant="main")
        other = opp.engine(G, S, **{k: v for k, v in sp._engine_args.items()
                                    if k not in ("fast_simulations", "full_search_prob")})
        c0 = sp.engine.counters()
        sp.reset()
        sp.engine.arena_move(other, sp.max_moves)
        c1 = sp.engine.counters()
        assert c1["playing"] == 0 and c1["simulations"] - c0["simulations"] == (c1["moves"] - c0["moves"]) * S
        out.append([sp.engine.record(g) for g in range(G)])
    _same_records(*out)
    assert not any((r["flags"] & FAST).any() for r in out[0]) and sum(r["length"] for r in out[0]) > G


# ---------------------------------------------------------------------------
# 4. against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_capped_games_match_the_oracle_move_for_move():
    """tests/test_gpu_selfplay.py::test_fixed_compat_games_match_oracle's method, the oracle
    agent built per move with that move's budget."""
    import mzgo
    from oracle import gogame as gg
    from oracle.net import OracleNet
    from oracle.rng import SearchHooks
    from oracle.selfplay import Agent
    from oracle.weights import deterministic_state_dict
    N, G, S, F, seed = _case("5x5")
    A, C = N * N + 1, 96
    sp = _selfplay("5x5")
    drawn = torch.zeros(G, sp.max_moves, A, dtype=torch.float64, device="cuda")
    sp.engine.record_noise(drawn)
    try:
        hists = sp.play()                      # epoch 0: game ids 0 .. G-1 key the streams
    finally:
        sp.engine.record_noise(None)
    drawn = drawn.cpu().numpy()
    onet = OracleNet(deterministic_state_dict(C, A, 0))
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    n_fast = n_full = 0
    try:
        for g, h in enumerate(hists):
            want = budgets(seed, g, len(h), S, F, GPU_P)
            assert h.fast_search == [b == F for b in want]
            st = gg.init_state(N)
            for mv, (obs, a, pol, v) in enumerate(zip(h.observations, h.actions, h.policies, h.values)):
                np.testing.assert_array_equal(obs, st)
                nz = drawn[g, mv]
                agent = Agent(onet, N, A, want[mv], compat="fixed",
                              noise=lambda p, act, e, nz=nz: (1 - e) * p + e * nz)
                oa, opol, oval = agent.select_action(obs, 1.0 if mv < 15 else 0, SearchHooks(seed, g, mv))
                assert a == oa, (g, mv, a, oa)
                assert pol.tobytes() == np.asarray(opol, np.float64).tobytes(), (g, mv)
                assert abs(v - oval) < 1e-5, (g, mv, v, oval)
                n_fast += want[mv] == F
                n_full += want[mv] == S
                st = gg.next_state(st, a)
    finally:
        torch.set_num_threads(nt)
    assert n_fast > 0 and n_full > 0


# ---------------------------------------------------------------------------
# 5. the three engines agree under caps
# ---------------------------------------------------------------------------
def _assert_same_game(got, want):
    assert got.keys() == want.keys()
    assert got["actions"] == want["actions"] and got["key_gid"] == want["key_gid"]
    assert got.get("fast_search") == want.get("fast_search")
    for a, b in zip(got["observations"], want["observations"]):
        np.testing.assert_array_equal(a, b)
    for k in ("rewards", "policies", "root_values"):
        np.testing.assert_array_equal(np.array(got[k], dtype=np.float64).view(np.uint64),
                                      np.array(want[k], dtype=np.float64).view(np.uint64), err_msg=k)


@pytest.mark.parametrize("name", ["6x6main", "9x9"])
def test_the_game_schedules_agree_under_caps(name):
    import mzgo
    from mzgo.replay import queue_key_gids
    N, G, S, F, seed = _case(name)
    if name == "6x6main":
        net = _net(N, 128, 5)
        make = lambda: _main_selfplay(net).sp
    else:
        net = _net(N)
        make = lambda: _selfplay(name, net, max_moves=14)
    sp = make()                                # (one engine: net.engine caches it per configuration)
    # per-move launches against one whole-game launch
    (ra, ca), (rb, cb) = _play(sp, per_move=True), _play(sp)
    _same_records(ra, rb)
    assert ca == cb
    n_fast, n_full, total = _check_flags(sp, rb, S, F)
    assert n_fast > 0 and n_full > 0 and cb["simulations"] == total
    # whole-game launches, ingested round by round, against the game queue
    n = 2 * G + 1
    want = mzgo.DeviceReplay(N, 3 * G, sp.max_moves, "cuda")
    for e in range(3):
        _play(sp, epoch=e)
        want.add_games(sp.engine)
    rp = mzgo.DeviceReplay(N, n, sp.max_moves, "cuda")
    c0 = sp.engine.counters()
    sp.epoch = 0
    sp.play_games_into(rp, n)
    c1 = sp.engine.counters()
    assert rp.lengths == want.lengths[:n] and rp.key_gids == want.key_gids[:n]
    assert rp.key_gids == [int(x) for x in queue_key_gids(n, G, 0, 0)]
    sims = fast_games = 0
    for j in range(n):
        got = rp.export(j)
        _assert_same_game(got, want.export(j))
        b = budgets(seed, got["key_gid"] & 0xFFFFFFFF, len(got["actions"]), S, F, GPU_P)
        assert got.get("fast_search", [False] * len(b)) == [x == F for x in b]
        fast_games += "fast_search" in got
        sims += sum(b)
    assert fast_games > 0
    assert c1["simulations"] - c0["simulations"] == sims and c1["moves"] - c0["moves"] == sum(rp.lengths)


@pytest.mark.parametrize("name", ["9x9", "19x19"])
def test_move_parallel_launch_equals_game_per_workgroup_under_caps(name, monkeypatch):
    N, G, S, F, seed = _case(name)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MZGO_MOVE_PARALLEL", mode)
        monkeypatch.setenv("MZGO_TAIL_HELPERS", "0")
        # (a net per mode: an engine of its own, made under the mode's environment)
        sp = _selfplay(name, _net(N), compat="reference", max_moves=12)
        out[mode] = (sp,) + _play(sp)
    (spa, ra, ca), (spb, rb, cb) = out["1"], out["0"]
    assert spa.engine is not spb.engine
    _same_records(ra, rb)
    assert ca == cb
    n_fast, n_full, total = _check_flags(spa, ra, S, F)
    assert n_fast > 0 and n_full > 0 and ca["simulations"] == total


# ---------------------------------------------------------------------------
# 6. the store masks and reanalysis unmasks
# ---------------------------------------------------------------------------
def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32) if t.dtype == torch.float32 else t.cpu().numpy()


def _capped_store(n=None):
    import mzgo
    msp = _main_selfplay()
    n = n or 2 * msp.sp.G + 1
    rp = mzgo.DeviceReplay(msp.N, n, msp.max_moves, "cuda")
    msp.play_games_into(rp, n)
    return msp, rp


def _stripped_copy(rp, games):
    """The store's games with bit 3 cleared: export -> strip the key -> add."""
    import mzgo
    cp = mzgo.DeviceReplay(rp.N, rp.capacity, rp.max_moves, "cuda")
    for g in games:
        cp.add({k: v for k, v in g.items() if k != "fast_search"}, key_gid=g["key_gid"])
    return cp


def test_store_masks_fast_rows_and_the_host_builder_agrees():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    K, td, d = 3, 2, 0.997
    msp, rp = _capped_store()
    games = [rp.export(j) for j in range(len(rp))]
    assert all("fast_search" in g for g in games)
    cp = _stripped_copy(rp, games)
    assert not any("fast_search" in cp.export(j) for j in range(len(cp)))
    A = rp.A
    idx = [j for j in range(len(rp)) for _ in range(3)]
    starts = [s for g in games for s in (0, len(g["actions"]) - 1, len(g["actions"]) // 2)]
    for sym in (None, [(3 * b + 1) % 8 for b in range(len(idx))]):
        for got, want in ((rp.batch(idx, starts, K, d, sym), cp.batch(idx, starts, K, d, sym)),
                          (rp.batch_values(idx, starts, K, td, d, sym), cp.batch_values(idx, starts, K, td, d, sym))):
            assert got.keys() == want.keys()
            for k in got:
                if k != "t_pol":
                    assert torch.equal(got[k], want[k]), k
            tp, wp = _u32(got["t_pol"]), _u32(want["t_pol"])
            zero = kept = past = 0
            for b, (j, s) in enumerate(zip(idx, starts)):
                L = len(games[j]["actions"])
                for k in range(K + 1):
                    i = s + k
                    if i < L and games[j]["fast_search"][i]:
                        assert not tp[b, k].any(), (b, k)
                        assert wp[b, k].any()
                        zero += 1
                    else:
                        np.testing.assert_array_equal(tp[b, k], wp[b, k])
                        kept += i < L
                        past += i >= L
                        if i >= L:
                            assert (tp[b, k] == np.float32(1.0 / A).view(np.uint32)).all()
            assert zero and kept and past
    # the host builder forms the device assembly's bits from the exported trajectories
    tr = MuZeroTrainer(msp.sp.net, TrainConfig(unroll_steps=K, discount=d), mode="batched")
    host = tr.batch_targets([games[j] for j in idx], starts)
    dev = rp.batch(idx, starts, K, d)
    np.testing.assert_array_equal(host[4].astype(np.float32).view(np.uint32), _u32(dev["t_pol"]))
    np.testing.assert_array_equal(host[3].astype(np.float32).view(np.uint32), _u32(dev["t_rew"]))
    np.testing.assert_array_equal(host[1], dev["acts"].cpu().numpy())


def test_reanalysis_into_the_store_clears_the_flag():
    from mzgo.reanalyse import Reanalyser
    K = 3
    msp, rp = _capped_store()
    N, G, S, F, seed = _case("6x6main")
    ra = Reanalyser(msp.sp.net, S, slots=4, seed=seed)
    before = [rp.export(j) for j in range(len(rp))]
    triples = [(j, s, 0) for j, g in enumerate(before) for s in (0, len(g["actions"]) - 2)][:8]
    items = torch.tensor(triples, dtype=torch.int32, device="cuda")
    inside = {(int(s), int(t)) for s, t in rp.window_items_host(items, K)}
    n = rp.reanalyse_sample(ra, items, K)
    assert n.item() == len(rp.window_items_host(items, K)) > 0
    after = [rp.export(j) for j in range(len(rp))]
    cleared = kept = 0
    for j, (a, b) in enumerate(zip(after, before)):            # (no wrap: slot = logical index)
        fa = a.get("fast_search", [False] * len(a["actions"]))
        for t, was in enumerate(b["fast_search"]):
            if (j, t) in inside:
                assert not fa[t] and np.any(a["policies"][t] != 0), (j, t)
                cleared += was
            else:
                assert fa[t] == was, (j, t)
                assert a["policies"][t].tobytes() == b["policies"][t].tobytes()
                assert a["root_values"][t] == b["root_values"][t]
                kept += was
        assert a["actions"] == b["actions"]
        for x, y in zip(a["observations"], b["observations"]):
            np.testing.assert_array_equal(x, y)                  # bits 0-2 stay
    assert cleared > 0 and kept > 0
    # the windows' rows are targets again: the batch reads them unmasked
    idx, starts = [t[0] for t in triples], [t[1] for t in triples]
    tp = rp.batch(idx, starts, K, 0.997)["t_pol"].cpu().numpy()
    for b, (j, s) in enumerate(zip(idx, starts)):
        for k in range(K + 1):
            if s + k < len(before[j]["actions"]):
                assert tp[b, k].any(), (b, k)
    # whole-game reanalysis (the staged path) leaves no fast row; a full row's search is its own again
    rp.reanalyse(ra)
    torch.cuda.synchronize()
    for j, b in enumerate(before):
        a = rp.export(j)
        assert "fast_search" not in a
        for t, was in enumerate(b["fast_search"]):
            assert np.any(a["policies"][t] != 0)
            if not was:
                assert a["root_values"][t] == b["root_values"][t], (j, t)


def test_host_reanalysis_unmasks_too():
    """``Reanalyser.run`` searches every move with the full budget: its trajectories name no fast move, so the
    host builder and ``DeviceReplay.add`` treat every row as a target again."""
    from mzgo.reanalyse import Reanalyser
    N, G, S, F, seed = _case("6x6main")
    msp, rp = _capped_store(3)
    games = [rp.export(j) for j in range(3)]
    assert all("fast_search" in g for g in games)
    fresh = Reanalyser(msp.sp.net, S, slots=4, seed=seed).run(games, ids=None)
    assert all("fast_search" in g for g in games)                # (the inputs stay as they were)
    for g, f in zip(games, fresh):
        assert "fast_search" not in f and f["actions"] == g["actions"]
        assert all(np.any(p != 0) for p in f["policies"])
    cp = _stripped_copy(rp, fresh)
    assert not any("fast_search" in cp.export(j) for j in range(3))


# ---------------------------------------------------------------------------
# 7. one trainer step
# ---------------------------------------------------------------------------
def test_one_trainer_step_from_a_capped_store():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    B, K = 8, 3
    msp, rp = _capped_store()
    A = rp.A
    net = mzgo.MuZeroNet(128, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(128, A, 6))
    cfg = TrainConfig(learning_rate=1e-3, unroll_steps=K, fused_loss=True, fused_unroll=True, device_sampling=True)
    tr = MuZeroTrainer(net, cfg, mode="batched", sample_seed=5)
    # the step's batch and the heads' outputs under the weights it starts from
    s = rp.sample_batch(B, K, cfg.discount, seed=5, step=0, symmetries=cfg.symmetries)
    t_pol = s["t_pol"].cpu().numpy()
    masked = ~t_pol.reshape(B, K + 1, A).any(-1)
    assert masked.any() and not masked.all()
    seen = {}
    import mzgo.loss as ml
    loss = ml.unroll_loss

    def spy(logits, value, reward, tp, tv, trw, **kw):
        seen.update(logits=logits.detach().cpu().numpy(), value=value.detach().cpu().numpy(),
                    reward=reward.detach().cpu().numpy(), t_pol=tp.cpu().numpy(), t_val=tv.cpu().numpy(),
                    t_rew=trw.cpu().numpy(), kw=kw)
        return loss(logits, value, reward, tp, tv, trw, **kw)

    ml.unroll_loss = spy                       # (the trainer imports it from the module at each step)
    try:
        assert tr.train(rp, B) is not None
    finally:
        ml.unroll_loss = loss
    stats = dict(tr.read_stats())
    for k in ("training_loss", "value_loss", "policy_loss", "reward_loss"):
        assert np.isfinite(stats[k]), (k, stats)
    np.testing.assert_array_equal(seen["t_pol"].view(np.uint32), t_pol.view(np.uint32))       # the batch drawn above
    # the policy total is the unmasked rows' alone: recomputed on the host with the masked rows' logits replaced
    host = mzgo.unroll_loss_host(seen["logits"], seen["value"], seen["reward"], seen["t_pol"], seen["t_val"],
                                 seen["t_rew"], **seen["kw"])
    scrambled = seen["logits"].copy()
    scrambled[masked.T] = np.random.RandomState(1).randn(int(masked.sum()), A).astype(np.float32)
    host2 = mzgo.unroll_loss_host(scrambled, seen["value"], seen["reward"], seen["t_pol"], seen["t_val"],
                                  seen["t_rew"], **seen["kw"])
    assert host[1][2] == host2[1][2]                             # masked rows add nothing, whatever the logits
    assert not host[2][masked.T].any()
    assert stats["policy_loss"] * B == pytest.approx(host[1][2], rel=1e-5)
